"""Exact-arithmetic probe nets for the fused ResNet (csrc/resnet.hip).

Ordinary AlphaZeroNet state dicts (keys as othello_mcts.synthetic
.alphazero_state_dict) whose forward pass the bf16 / fp16 kernel computes
WITHOUT any rounding: every folded conv weight and bias is a small integer,
the inputs are 0/1 planes and no value the kernel holds between layers exceeds
256 (exact in bf16; fp16 is exact to 2048). The heads' fp32 sums are exact in
any summation order (every term is an integer multiple of one power of two
and the terms' magnitudes sum to less than 2^24 such units). One wrong unit
anywhere in the tower therefore moves a logit by at least one `step`, and the
comparison allows a quarter of a step.

Two families:
  * routing nets (family "A"): every output channel of every 3x3 conv reads
    ONE (input channel, tap), through a per-layer channel permutation and a
    tap that varies with channel and layer: they exercise every address map
    (K order, out_chan, kgroup_chunk, tile position maps, border handling).
  * integer nets (family "B"): random ternary 3x3 convs summing many K entries
    per output, with non-trivial BatchNorm that still folds exactly: they
    exercise accumulation (a K-step counted twice or never, a stale weight
    slot) and the loader's BN fold.
The head parameters are calibrated on the reference's own outputs over the
master input batch (never on the kernel's): ReLU thresholds at a quantile and
the power-of-two scales that keep the 65 logits within a spread of 16 and the
value pre-activation within +-3.

forward_exact is the integer reference. It is linked to the fp32 torch
restatement (oracle/resnet_ref.py) in tests/test_cpu_exact_nets.py.

These nets avoid rounding on purpose: they prove addressing and accumulation.
Which number the kernel's epilogue and the loader round to is pinned, with the
same comparison, by the third family in tests/rounding_nets.py (nets whose
layer results do not fit the 16-bit format); how large the rounding error of
a live net is stays with the tolerance tests of tests/test_gpu_resnet.py.
"""

from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from othello_mcts.synthetic import portable_uniform

BN_EPS = 1e-5
U_MAX = 256              # integers up to 256 are exact in bf16 (8 significant bits)
SUM_BOUND = float(1 << 24)
MAX_SPREAD = 16.0        # logit spread: every probability a normal fp32 number
MAX_Z = 3.0
MIN_QUARTER_STEP = 1e-4  # ~50x the fp32 softmax / tanhf deviation at these magnitudes
MASTER_ROWS = 1027       # every batch the tests use is a prefix of the master batch
VAR1 = np.float32(1.0 - 1e-5)  # + eps = 1 to 3e-8: the folded scale is 1 +- 2e-8
VAR4 = np.float32(4.0 - 1e-5)  # ... one half


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def inputs(cin: int) -> np.ndarray:
    """Master batch (MASTER_ROWS, cin, 8, 8) of distinct seeded 0/1 boards;
    plane 0 is constant per board (cin > 1); row 1 is all zeros, row 2 all ones."""
    u = portable_uniform(20261019, cin, MASTER_ROWS * cin * 64).reshape(MASTER_ROWS, cin, 8, 8)
    x = (u < 0.3).astype(np.float32)
    if cin > 1:  # a single plane has to tell the boards apart itself
        x[:, 0] = (u[:, 0, :1, :1] < 0.5).astype(np.float32)
    x[1] = 0.0
    x[2] = 1.0
    assert len({r.tobytes() for r in x}) == MASTER_ROWS
    x.setflags(write=False)
    return x


# ------------------------------------------------------------------ builders
def _put_conv(sd, p, w, b=None):
    sd[p + ".weight"] = np.ascontiguousarray(w, dtype=np.float32)
    sd[p + ".bias"] = np.zeros(w.shape[0], np.float32) if b is None else np.asarray(b, np.float32)


def _put_bn(sd, p, beta, gamma=None, mean=None, var=None):
    beta = np.asarray(beta, np.float32)
    n = beta.shape[0]
    sd[p + ".weight"] = np.ones(n, np.float32) if gamma is None else np.asarray(gamma, np.float32)
    sd[p + ".bias"] = beta
    sd[p + ".running_mean"] = np.zeros(n, np.float32) if mean is None else np.asarray(mean, np.float32)
    sd[p + ".running_var"] = np.full(n, VAR1, np.float32) if var is None else np.asarray(var, np.float32)
    sd[p + ".num_batches_tracked"] = np.array(0, dtype=np.int64)


def _routing_conv(C, cin, src, tap, sign):
    w = np.zeros((C, cin, 3, 3), np.float32)
    w[np.arange(C), src, tap // 3, tap % 3] = sign
    return w


def routing_tower(C: int, R: int, cin: int, phase: int) -> dict:
    """Family A tower. Block l: conv1 reads channel (5 co + 3 l + 1) mod C at
    tap (co + l) mod 9 with weight +1; conv2 reads (3 co + 7 l + 2) mod C at
    tap (2 co + l + 4) mod 9 with weight +1 / -1 / 0 / 0 by (co + l + phase)
    mod 4. First conv: plane co mod cin at tap (co + co // cin) mod 9. All
    biases are zero (the integer nets carry the biases): with them every
    channel of the 128x9b tower's output is non-zero on more than a fifth of
    the squares and U is 8-21 there, 22-202 for 256x19b (phases 1 and 3 grow);
    negative biases were tried and left a quarter of the channels dead after
    nine blocks."""
    sd: dict = {}
    co = np.arange(C)
    _put_conv(sd, "conv_block.conv", _routing_conv(C, cin, co % cin, (co + co // cin) % 9, 1.0))
    _put_bn(sd, "conv_block.norm", np.zeros(C))
    for l in range(R):
        p = f"residual_blocks.{l}"
        _put_conv(sd, p + ".conv1", _routing_conv(C, C, (5 * co + 3 * l + 1) % C, (co + l) % 9, 1.0))
        _put_bn(sd, p + ".norm1", np.zeros(C))
        sign = np.array([1.0, -1.0, 0.0, 0.0])[(co + l + phase) % 4]
        _put_conv(sd, p + ".conv2", _routing_conv(C, C, (3 * co + 7 * l + 2) % C, (2 * co + l + 4) % 9, sign))
        _put_bn(sd, p + ".norm2", np.zeros(C))
    return sd


# family B: share of non-zero ternary weights and the bias base per conv layer
# (first conv, then the blocks' convs). Only the first conv is 25 % dense. A
# 3x3 conv with n weights +-1 per output multiplies the spread of its input by
# about sqrt(n q), q = the rectified input's second moment over its variance
# (0.04 for a normal variable with 10 % above the threshold, more for these
# heavier tails), so at n = 9 C / 4 the spread would grow more than 3x per
# conv and leave U <= 256 within the five convs of R = 2 even from a first
# conv of spread 3. The tower's convs keep n = 9 C d of 24-34: every
# K-step (one tap x 32 channels) still carries 80-120 non-zero weights, so a
# K-step counted twice or never changes outputs at every position. Measured
# on the master batch: U = 215 (C=128) and 198 (C=256).
INTEGER_DENSITY = {128: (0.25, 0.03, 0.02, 0.02, 0.02), 256: (0.25, 0.015, 0.01, 0.01, 0.01)}
INTEGER_BIAS = {128: (2, 3, 4, 7, 10), 256: (2, 3, 4, 6, 11)}


def integer_tower(C: int, R: int, cin: int, seed: int = 7) -> dict:
    """Family B tower (R <= 2): random ternary weights, folded bias
    -(base + c mod 3), and per channel c one of four BatchNorms that fold
    exactly: (gamma, var) = (1, 1), (2, 4), (0.5, 1), (1, 4) (scale 1, 1, 1/2,
    1/2; the raw weights of the half-scale channels are +-2), integer running
    mean and a non-zero conv bias."""
    assert R <= 2
    sd: dict = {}
    c = np.arange(C)
    kind = c % 4
    gamma = np.array([1.0, 2.0, 0.5, 1.0])[kind]
    var = np.where((kind == 1) | (kind == 3), VAR4, VAR1)
    scale = np.array([1.0, 1.0, 0.5, 0.5])[kind]
    # non-zero conv bias cb and integer running mean mu with cb - mu in {-2, 0,
    # 2}: the fold (cb - mu) * scale + beta carries the scale's 1.5e-8 relative
    # error times |cb - mu|, which must stay below half an ulp of the folded
    # bias (|bias| >= 2: 1.2e-7)
    cb = 1.0 + c % 2
    mu = cb - 2.0 * ((c // 4) % 3 - 1)
    names = [("conv_block.conv", "conv_block.norm")]
    for l in range(R):
        names += [(f"residual_blocks.{l}.conv1", f"residual_blocks.{l}.norm1"),
                  (f"residual_blocks.{l}.conv2", f"residual_blocks.{l}.norm2")]
    for layer, (pc, pn) in enumerate(names):
        ci = cin if layer == 0 else C
        d = INTEGER_DENSITY[C][layer]
        w = _balanced(seed, 100 * C + layer, C, ci * 9, max(1, round(d * ci * 9 / 2))).reshape(C, ci, 3, 3)
        want_bias = -(INTEGER_BIAS[C][layer] + c % 3).astype(np.float64)
        _put_conv(sd, pc, w / scale[:, None, None, None], cb)
        _put_bn(sd, pn, want_bias - (cb - mu) * scale, gamma, mu, var)
    return sd


def _balanced(seed, stream, rows, cols, n):
    """(rows, cols) ternary: every row has n weights +1 and n weights -1 at
    seeded random places (balanced, so an offset common to a row's inputs
    cancels)."""
    order = np.argsort(portable_uniform(seed, stream, rows * cols).reshape(rows, cols), axis=1, kind="stable")
    w = np.zeros((rows, cols))
    np.put_along_axis(w, order[:, :n], 1.0, axis=1)
    np.put_along_axis(w, order[:, n:2 * n], -1.0, axis=1)
    return w


def _ternary(seed, stream, shape, nonzero):
    u = portable_uniform(seed, stream, int(np.prod(shape))).reshape(shape)
    return np.where(u < nonzero / 2, -1.0, np.where(u < nonzero, 1.0, 0.0))


def _pow2_scale(extent: float, limit: float) -> float:
    """Largest 2^-k (k >= 0) with extent * 2^-k <= limit."""
    k = 0
    while extent * 2.0 ** -k > limit:
        k += 1
    return 2.0 ** -k


def add_heads(sd: dict, h: np.ndarray, hid: int, seed: int = 11) -> dict:
    """Heads for a tower whose exact output over the master batch is h
    (C, N, 64). The 1x1 convs read every channel with small integer weights
    whose magnitudes differ between neighbouring channels and across groups
    of 4, 8, 16 and 32 (periods 5, 7 and 3) and whose seeded signs keep a
    board-wide offset of the tower output from piling up (all-positive weights
    cost a factor 8 in step); ReLU thresholds at the median (policy) and the
    90th percentile (value) of the master batch. Policy Linear: ternary, a
    quarter non-zero, x 2^-k, action 64 included. Value:
    Linear(64 -> hid) with three weights +1 and three -1 per unit,
    thresholded per unit at its 60th percentile; Linear(hid -> 1) with
    weights +1, -1 alternating (every unit counts, neighbours differ), x 2^-k."""
    C, N, _ = h.shape
    c = np.arange(C)
    sign = np.where(portable_uniform(seed, 0, 3 * C).reshape(3, C) < 0.5, -1, 1)
    hw = (sign * np.stack([1 + (7 * c) % 5, 1 + (3 * c) % 7, 1 + (2 * c) % 3])).astype(np.float32)
    pre = (hw @ h.reshape(C, -1).astype(np.float32)).reshape(3, N, 64).astype(np.float64)
    hb = -np.floor([np.quantile(pre[0], 0.5), np.quantile(pre[1], 0.5), np.quantile(pre[2], 0.9)])
    act = np.maximum(pre + hb[:, None, None], 0.0)
    _put_conv(sd, "policy_head.conv", hw[:2].reshape(2, C, 1, 1))
    _put_bn(sd, "policy_head.norm", hb[:2])
    _put_conv(sd, "value_head.conv", hw[2:].reshape(1, C, 1, 1))
    _put_bn(sd, "value_head.norm", hb[2:])
    # policy: logits = T flat + t, flat index = channel * 64 + square
    T = _ternary(seed, 1, (65, 128), 0.25)
    t = np.round(4.0 * portable_uniform(seed, 2, 65)) - 2.0
    flat = act[:2].transpose(1, 0, 2).reshape(N, 128)
    L = flat @ T.T + t
    s = _pow2_scale(float((L.max(1) - L.min(1)).max()), MAX_SPREAD)
    sd["policy_head.linear.weight"] = (T * s).astype(np.float32)
    sd["policy_head.linear.bias"] = (t * s).astype(np.float32)
    # value
    W1 = _balanced(seed, 3, hid, 64, 3)
    A = act[2] @ W1.T  # (N, hid)
    b1 = -np.floor(np.quantile(A, 0.6, axis=0))
    H = np.maximum(A + b1, 0.0)
    w2 = np.array([1.0, -1.0])[np.arange(hid) % 2]
    z = H @ w2
    b2 = -np.round(np.median(z))
    sv = _pow2_scale(float(np.abs(z + b2).max()), MAX_Z)
    sd["value_head.linear1.weight"] = W1.astype(np.float32)
    sd["value_head.linear1.bias"] = b1.astype(np.float32)
    sd["value_head.linear2.weight"] = (w2 * sv).reshape(1, hid).astype(np.float32)
    sd["value_head.linear2.bias"] = np.array([b2 * sv], np.float32)
    return sd


# ------------------------------------------------------------------ the loader's fold, restated
def _round_to(a: np.ndarray, dtype: str) -> np.ndarray:
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return t.to(torch.bfloat16 if dtype == "bf16" else torch.float16).to(torch.float32).numpy()


def fold(sd: dict, conv: str, norm: str) -> tuple[np.ndarray, np.ndarray]:
    """Folded (weight, bias) of conv + BatchNorm as oamd_net_load_state computes
    them: in double with eps 1e-5, cast to float32."""
    g = sd[norm + ".weight"].astype(np.float64)
    scale = g / np.sqrt(sd[norm + ".running_var"].astype(np.float64) + BN_EPS)
    w = (sd[conv + ".weight"].astype(np.float64) * scale.reshape(-1, 1, 1, 1)).astype(np.float32)
    b = ((sd[conv + ".bias"].astype(np.float64) - sd[norm + ".running_mean"].astype(np.float64)) * scale
         + sd[norm + ".bias"].astype(np.float64)).astype(np.float32)
    return w, b


def _folded_integers(sd, conv, norm):
    """The folded conv as int arrays, asserting the exactness rules: integer
    weights with |w| <= 8 that both 16-bit formats hold unchanged (the loader
    rounds float32 -> bf16 RNE / fp16), integer bias."""
    w, b = fold(sd, conv, norm)
    assert np.array_equal(w, np.rint(w)) and np.abs(w).max() <= 8, f"{conv}: folded weights are not integers <= 8"
    assert np.array_equal(b, np.rint(b)), f"{conv}: folded bias is not an integer"
    vals = np.unique(w)  # elementwise formats: the distinct values decide
    for dt in ("bf16", "fp16"):
        assert np.array_equal(_round_to(vals, dt), vals), f"{conv}: folded weights change in {dt}"
    return w.astype(np.int64), b.astype(np.int64)


def conv_layers(sd) -> list[tuple[str, str]]:
    out = [("conv_block.conv", "conv_block.norm")]
    i = 0
    while f"residual_blocks.{i}.conv1.weight" in sd:
        out += [(f"residual_blocks.{i}.conv1", f"residual_blocks.{i}.norm1"),
                (f"residual_blocks.{i}.conv2", f"residual_blocks.{i}.norm2")]
        i += 1
    return out


# ------------------------------------------------------------------ exact tower
def _conv_exact(w, a):
    """3x3 'same' convolution of a (Cin, N, 8, 8) int16 by integer weights
    w (Cout, Cin, 3, 3), exactly, as int16 or int32 (Cout, N, 8, 8). A conv whose output
    channels each read at most one (channel, tap) is gathered and shifted; any
    other runs as a float32 convolution whose sums stay below 2^24."""
    cout, cin = w.shape[:2]
    n = a.shape[1]
    wf = w.reshape(cout, -1)
    if (wf != 0).sum(1).max() <= 1:
        pad = np.zeros((cin, n, 10, 10), np.int16)
        pad[:, :, 1:9, 1:9] = a
        out = np.zeros((cout, n, 8, 8), np.int16)  # |w| <= 8, |a| <= 256: no overflow
        idx = np.abs(wf).argmax(1)
        val = wf[np.arange(cout), idx]
        src, tap = idx // 9, idx % 9
        for t in range(9):
            ky, kx = divmod(t, 3)
            for v in np.unique(val[(tap == t) & (val != 0)]):
                cs = np.nonzero((tap == t) & (val == v))[0]
                g = pad[src[cs], :, ky:ky + 8, kx:kx + 8]
                out[cs] = g if v == 1 else g * np.int16(v)
        return out
    import torch
    import torch.nn.functional as F

    assert np.abs(wf).sum(1).max() * max(int(np.abs(a).max()), 1) < SUM_BOUND, "dense conv: sums leave 2^24"
    y = F.conv2d(torch.from_numpy(a.transpose(1, 0, 2, 3).astype(np.float32)),
                 torch.from_numpy(w.astype(np.float32)), padding=1)
    return np.rint(y.numpy()).astype(np.int32).transpose(1, 0, 2, 3)


def tower_exact(sd, x, drop_skip=None, swap_out=None):
    """Exact tower of sd on 0/1 planes x (N, cin, 8, 8): its output (C, N, 64)
    int16, U = the largest |value| held between layers (pre-ReLU conv outputs,
    residual sums, activations), and the non-zero share of every conv layer's
    rectified output. Mutations for the tests of the tests: drop_skip = a
    block whose skip is left out; swap_out = (conv layer, i, j) stores that
    layer's output channels i and j in each other's place."""
    assert np.isin(x, (0.0, 1.0)).all()
    a = np.ascontiguousarray(x.transpose(1, 0, 2, 3)).astype(np.int16)
    U, fracs, skip = 1, [], None
    for layer, (pc, pn) in enumerate(conv_layers(sd)):
        w, b = _folded_integers(sd, pc, pn)
        assert a.max(initial=0) <= U_MAX and a.min(initial=0) >= 0 and np.abs(b).max() <= 4096
        y = _conv_exact(w, a)
        y += b[:, None, None, None].astype(y.dtype)
        second = layer > 0 and layer % 2 == 0
        if layer % 2 == 1:
            skip = a
        if second and drop_skip != (layer - 2) // 2:
            # the kernel starts its accumulators at bias + skip: that sum and
            # the total are both held in fp32 and stay far below 2^24; only
            # the stored result must be exact in 16 bits
            y += skip
        U = max(U, int(y.max()), -int(y.min()))
        assert U <= U_MAX, f"{pc}: |value| {U} > {U_MAX} is not exact in bf16"
        a = np.maximum(y, 0, out=y).astype(np.int16, copy=False)
        if swap_out is not None and swap_out[0] == layer:
            a[[swap_out[1], swap_out[2]]] = a[[swap_out[2], swap_out[1]]]
        fracs.append(float(np.count_nonzero(a)) / a.size)
    return a.reshape(a.shape[0], a.shape[1], 64), U, fracs


def _quantum(*arrays) -> float:
    """Largest power of two of which every entry of the arrays is a multiple."""
    q = 1.0
    for _ in range(40):
        if all(np.array_equal(np.asarray(a, np.float64) / q, np.rint(np.asarray(a, np.float64) / q)) for a in arrays):
            return q
        q /= 2
    raise AssertionError("weights are not small integers times a power of two")


def _affine_exact(name, W, b, X, qx=1.0):
    """Y = X W^T + b in float64 and Y's quantum; asserts that the fp32 sum is
    exact in any order: in units of the terms' common quantum, the magnitudes
    of the terms (bias included) sum to less than 2^24."""
    W = np.asarray(W, np.float64)
    b = np.asarray(b, np.float64)
    q = _quantum(W, b / qx) * qx
    mag = np.abs(X) @ np.abs(W).T + np.abs(b)
    assert mag.max() / q < SUM_BOUND, f"{name}: sum of |terms| = {mag.max() / q:.3g} quanta >= 2^24"
    return X @ W.T + b, q


@dataclass
class Reference:
    logits: np.ndarray   # (N, 65) float64, exact
    z: np.ndarray        # (N,) value pre-activation, exact
    U: int
    fracs: list
    step: float          # the logits' quantum: the least change one wrong tower unit causes
    step_v: float        # ... of z

    def rows(self, n: int) -> "Reference":
        return Reference(self.logits[:n], self.z[:n], self.U, self.fracs, self.step, self.step_v)


def heads_exact(sd, h, U=0, fracs=()):
    """The heads of sd on an exact tower output h (C, N, 64)."""
    C, N, _ = h.shape
    wp, bp = _folded_integers(sd, "policy_head.conv", "policy_head.norm")
    wv, bv = _folded_integers(sd, "value_head.conv", "value_head.norm")
    hw = np.concatenate([wp.reshape(2, C), wv.reshape(1, C)]).astype(np.float64)
    hb = np.concatenate([bp, bv]).astype(np.float64)
    assert (np.abs(hw).sum(1) * max(int(np.abs(h).max()), 1) + np.abs(hb)).max() < SUM_BOUND, "head conv sums"
    pre = (hw.astype(np.float32) @ h.reshape(C, -1).astype(np.float32)).reshape(3, N, 64).astype(np.float64)
    act = np.maximum(pre + hb[:, None, None], 0.0)
    flat = act[:2].transpose(1, 0, 2).reshape(N, 128)
    L, step = _affine_exact("policy_head.linear", sd["policy_head.linear.weight"], sd["policy_head.linear.bias"], flat)
    A, q1 = _affine_exact("value_head.linear1", sd["value_head.linear1.weight"], sd["value_head.linear1.bias"], act[2])
    z, step_v = _affine_exact("value_head.linear2", sd["value_head.linear2.weight"], sd["value_head.linear2.bias"],
                              np.maximum(A, 0.0), q1)
    return Reference(L, z[:, 0], U, list(fracs), step, step_v)


def forward_exact(sd, x, drop_skip=None, swap_out=None) -> Reference:
    """Exact forward of an exact net: the 65 logits, the value pre-activation z,
    U and the layers' non-zero shares; asserts the exactness rules."""
    h, U, fracs = tower_exact(sd, x, drop_skip, swap_out)
    return heads_exact(sd, h, U, fracs)


def outputs_of(ref: Reference) -> tuple[np.ndarray, np.ndarray]:
    """What a correct kernel returns for ref: float32 softmax and tanh."""
    e = np.exp(ref.logits - ref.logits.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)).astype(np.float32), np.tanh(ref.z).astype(np.float32)


def check_scales(ref: Reference) -> None:
    """The conditions under which the quarter-step tolerance is meaningful."""
    assert (ref.logits.max(1) - ref.logits.min(1)).max() <= MAX_SPREAD
    assert np.abs(ref.z).max() <= MAX_Z
    assert ref.step / 4 >= MIN_QUARTER_STEP and ref.step_v / 4 >= MIN_QUARTER_STEP


# ------------------------------------------------------------------ comparison
def deviations(policy, value, ref: Reference) -> dict:
    """Largest deviations of a kernel's (policy, value) from ref in the logit
    domain, in steps, with the row and action where the policy's occurs."""
    p = np.asarray(policy, np.float64)
    v = np.asarray(value, np.float64)
    assert p.shape == ref.logits.shape and v.shape == ref.z.shape
    with np.errstate(divide="ignore", invalid="ignore"):
        dl = np.abs(np.log(p / p[:, 64:65]) - (ref.logits - ref.logits[:, 64:65])) / ref.step
        dz = np.abs(np.arctanh(v) - ref.z) / ref.step_v
    dl = np.where(np.isfinite(dl), dl, np.inf)
    dz = np.where(np.isfinite(dz), dz, np.inf)
    row, action = np.unravel_index(int(dl.argmax()), dl.shape)
    return {"policy_steps": float(dl.max()), "row": int(row), "action": int(action),
            "value_steps": float(dz.max()), "value_row": int(dz.argmax()),
            "sum_err": float(np.abs(p.sum(1) - 1.0).max())}


def compare(policy, value, ref: Reference, label: str = "", report=None) -> dict:
    """Assert that (policy, value) is ref to a quarter of a step; report(d)
    sees the measured deviations first."""
    d = deviations(policy, value, ref)
    if report is not None:
        report(d)
    assert d["policy_steps"] <= 0.25, (f"{label}: policy logit off by {d['policy_steps']:.3g} steps "
                                       f"at row {d['row']} action {d['action']}")
    assert d["value_steps"] <= 0.25, f"{label}: value off by {d['value_steps']:.3g} steps at row {d['value_row']}"
    assert d["sum_err"] <= 1e-5, f"{label}: |sum p - 1| = {d['sum_err']:.3g}"
    return d


# ------------------------------------------------------------------ cases
@functools.lru_cache(maxsize=2)
def _tower(family: str, C: int, R: int, cin: int, phase: int):
    sd = routing_tower(C, R, cin, phase) if family == "A" else integer_tower(C, R, cin)
    return sd, tower_exact(sd, inputs(cin))


@functools.lru_cache(maxsize=2)
def case(family: str, C: int, R: int, cin: int = 17, hid: int = 64, phase: int = 0):
    """(state dict, master inputs, Reference over the master batch) of one net;
    a batch of n rows is inputs[:n] against reference.rows(n)."""
    tower, (h, U, fracs) = _tower(family, C, R, cin, phase if family == "A" else 0)
    sd = add_heads(dict(tower), h, hid)
    return sd, inputs(cin), heads_exact(sd, h, U, fracs)


# What tests/test_gpu_resnet_exact.py runs: (case arguments, row counts) per
# group. tests/test_cpu_exact_nets.py asserts the exactness conditions for
# exactly these. >= 1024 rows run the throughput geometries (4 boards per
# workgroup at C=128, 2 at C=256; 1027 = 4 x 256 + 3 and 1025 = 2 x 512 + 1
# leave the last workgroup ragged), fewer the one-board geometry.
BOARDS_PER_WG = {128: 4, 256: 2}
ROUTING = [(("A", C, R, 17, 64, phase), rows)
           for C, R, rows in ((128, 9, (5, 1027)), (256, 19, (3, 1025))) for phase in range(4)]
GEOMETRY = [(("A", C, 1, 17, 64, 0), (1, 2, 4, 7, 1023, 1024)) for C in (128, 256)]
DEPTH = [(("A", C, R, cin, 64, 0), (5, 1027)) for C in (128, 256) for R in (0, 1, 2) for cin in (1, 3, 31)]
HEADS = [(("A", C, 1, 17, hid, 0), (3, 1025)) for C in (128, 256) for hid in (1, 33, 64, 65, 100, 1024)]
INTEGER = [(("B", 128, 2, 17, 64, 0), (7, 1027)), (("B", 256, 2, 17, 64, 0), (7, 1025))]
ALL_CASES = ROUTING + GEOMETRY + DEPTH + HEADS + INTEGER


def case_id(args) -> str:
    family, C, R, cin, hid, phase = args
    return f"{family}-c{C}b{R}-in{cin}-hid{hid}" + (f"-ph{phase}" if family == "A" else "")
