"""Rounding probe nets for the fused ResNet (csrc/resnet.hip): the third probe
family beside tests/exact_nets.py's routing and integer nets.

Ordinary AlphaZeroNet state dicts (same keys) whose fp32 accumulation is exact
in every summation order, as in exact_nets (every term of a sum is an integer
multiple of one power of two, the layer's unit, and the terms' magnitudes sum
to less than 2^24 units), but whose per-layer results do NOT fit the storage
dtype: the value that reaches the epilogue needs more than 8 (bf16) or 11
(fp16) significant bits. What the kernel stores is then one specific rounded
number, which forward_rounded predicts bit for bit with an explicit integer
round-to-nearest-even, at any layer and in any geometry. One wrong rounding
moves a logit by at least one `step`; exact_nets.compare's quarter-step
criterion applies unchanged and no measured tolerance is involved.

The kernel's numeric spec, as read from csrc/capi_net.hip (oamd_net_load_state)
and csrc/resnet.hip (pack_relu, the accumulator start, heads()):
  * fold: scale = gamma / sqrt(var + 1e-5) in double; weight (float)(W scale),
    then rounded to the dtype (RNE); bias (float)((b - mu) scale + beta), kept
    in fp32 (exact_nets.fold restates the double -> float part);
  * tower: the fp32 accumulator starts from the folded bias, for a block's
    second conv plus the block's input as stored (already rounded); products
    accumulate in fp32; ONE RNE conversion to the dtype, then ReLU on the
    rounded value (negative results, -0 included, become +0);
  * heads: both 1x1 convs multiply dtype-rounded folded weights with the
    stored tower output into an fp32 accumulator from 0; the fp32 bias and
    ReLU follow; everything after is fp32.

Three families, one builder per dtype (what needs rounding differs, and fp16
has a ceiling: every fp16 pre-rounding magnitude stays at or below 2^15;
overflow and subnormals are out of scope):
  * "R" tower nets: integer weights, so every layer's unit is 1. The first
    conv has large integer weights the dtype holds (up to 128 / 2048) on 0/1
    inputs, so it rounds too; the later convs have few +-1 taps per output
    (the number is calibrated per layer so that the magnitudes stay in the
    band where the dtype rounds) and BatchNorms that fold exactly with scales
    1 and 1/2; the folded biases are negative odd integers of more than p
    significant bits.
  * "L" loader nets: routing-style towers whose raw fp32 weights times the
    BatchNorm scale give folded fp32 weights of p + 3 significant bits: the
    loader's float -> 16-bit rounding decides, ties both ways, a carry into
    the next binade, and channels where rounding the double product directly
    would differ from double -> float -> 16 bits.
  * "H" head-conv nets: an exact 0/1 tower under head 1x1 weights of p + 3
    significant bits.
The heads read the tower sparsely: a stored fp16 activation spans up to 2^15
units, and the 65 logits must fit a spread of 64 at a step of at least
4 x exact_nets.MIN_QUARTER_STEP, so each head conv row reads K channels (K is
the largest power of two that keeps the step; the channels rotate with the
case) and the value head looks at the value conv's output through a window
(ReLU(window - ReLU(pre - threshold)), exact and bounded).

Conditions asserted in the builders, per layer over the whole master batch:
the 2^24-unit bound (from above: the largest row sum of |w| times the largest
|a|, plus |bias| and |skip|), every value a multiple of the unit, normal
numbers the dtype holds, fp16 magnitudes <= 2^15. Coverage conditions of the
tower nets (coverage_failures), per conv layer and counted over the first
COVER_ROWS boards, so they are lower bounds for every large batch: >= 10 %
inexact pre-rounding values, >= 64 exact ties resolved each way, >= 64
inexact negatives, >= 64 values within one dtype ulp above zero and >= 64
within half an ulp below (the ulp at the layer's largest magnitude: the
grain the layer's rounding has; near zero the values themselves are exact),
and for second convs >= 64 values whose result depends on whether the skip
is added before the rounding.

Everything is calibrated on the reference's own outputs over the master batch
(never on the kernel's). tests/test_cpu_rounding_nets.py links forward_rounded
to torch's 16-bit casts and to oracle/resnet_ref.py and shows that the
comparison rejects the wrong rounding rules named there.
"""

from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import exact_nets as E
from othello_mcts.synthetic import portable_uniform

P_BITS = {"bf16": 8, "fp16": 11}             # significant bits
MIN_NORMAL = {"bf16": 2.0 ** -126, "fp16": 2.0 ** -14}
MAX_FINITE = {"bf16": 3.38e38, "fp16": 65504.0}
FP16_PRE_MAX = 2.0 ** 15                     # fp16: every pre-rounding magnitude stays below
# the builders keep every pre-rounding magnitude below this: the top of the
# band in which the dtype rounds integers (bf16 from 2^8, fp16 from 2^11)
BAND_TOP = {"bf16": 2.0 ** 13, "fp16": 0.9 * FP16_PRE_MAX}
FIRST_WMAX = {"bf16": 128, "fp16": 2048}     # first conv: integer weights up to this
FIRST_TAPS = {"bf16": 20, "fp16": 8}         # ... this many +, as many -, per output
# Logit spread of this family. Every probability stays a normal fp32 number
# (spread < 87), and the comparison's log(p / p64) carries at most
# 2 x 2^-23 (64 + 8) = 1.7e-5 of fp32 error (two probabilities, each of
# relative error 2^-23 (|o - m| + 8): __expf(d) is exp2 of the fp32 product
# d log2e, whose rounding and the constant's give 1.5 x 2^-24 |d|, plus a few
# ulps from exp2, the sum and the reciprocal): a sixth of the smallest quarter
# step exact_nets allows (MIN_QUARTER_STEP).
MAX_SPREAD = 64.0
COVER_MIN = 64                               # coverage conditions: at least this many of each kind
COVER_INEXACT = 0.10                         # ... and this share of inexact pre-rounding values
COVER_ROWS = 128                             # counted over the first boards of the master batch
MUTANTS = ("trunc", "away", "relu_late", "round_before_skip", "skip_unrounded", "w_trunc", "w_double",
           "head_fp32", "bias16")


# ------------------------------------------------------------------ explicit rounding
def _bits(y):
    y = np.ascontiguousarray(y, dtype=np.float64)
    return y, y.view(np.uint64)


def rne(y, p: int, mode: str = "rne") -> np.ndarray:
    """y rounded to p significant bits, in integer arithmetic on the bits of
    the float64 that holds y exactly (sign, exponent, 52-bit significand field;
    every y here is a normal float64 or zero): with d = 53 - p dropped bits,
    round to nearest with ties to even adds 2^(d-1) - 1 + (the lowest kept
    bit) and clears the d low bits ("rne"; a carry out of the significand
    field raises the exponent, as it must); ties away from zero adds 2^(d-1)
    ("away"); toward zero only clears ("trunc"). The sign bit is untouched
    (-0 stays -0)."""
    y, u = _bits(y)
    d = np.uint64(53 - p)
    one = np.uint64(1)
    if mode == "rne":
        u = u + ((one << (d - one)) - one + ((u >> d) & one))
    elif mode == "away":
        u = u + (one << (d - one))
    else:
        assert mode == "trunc"
    return (u & ~((one << d) - one)).view(np.float64).reshape(y.shape)


def ulp_of(v: float, p: int) -> float:
    """The spacing of p-bit numbers at magnitude v > 0."""
    return float(2.0 ** (np.floor(np.log2(v)) - p + 1))


def classify(y, p: int):
    """(inexact, tie resolved toward zero = down to even, tie resolved away
    from zero = up to even) masks of y at p significant bits."""
    y, u = _bits(y)
    d = np.uint64(53 - p)
    one = np.uint64(1)
    rem = u & ((one << d) - one)
    tie = rem == (one << (d - one))
    odd = ((u >> d) & one) == one
    return rem != 0, tie & ~odd, tie & odd


def representable(y, p: int) -> bool:
    y, u = _bits(y)
    return not (u & ((np.uint64(1) << np.uint64(53 - p)) - np.uint64(1))).any()


# ------------------------------------------------------------------ exact convolution
def conv3x3(w: np.ndarray, a: np.ndarray) -> np.ndarray:
    """3x3 'same' convolution of a (Cin, N, 64) float64 by w (Cout, Cin, 3, 3)
    float64, as (Cout, N, 64) float64: a float64 torch convolution, exact in
    any summation order whenever the caller's 2^24-unit bound holds (every
    partial sum is then an integer multiple of the unit below 2^53 units)."""
    import torch
    import torch.nn.functional as F

    cout, cin = w.shape[:2]
    n = a.shape[1]
    y = F.conv2d(torch.from_numpy(np.ascontiguousarray(a.reshape(cin, n, 8, 8).transpose(1, 0, 2, 3))),
                 torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)), padding=1)
    return np.ascontiguousarray(y.numpy().transpose(1, 0, 2, 3)).reshape(cout, n, 64)


# ------------------------------------------------------------------ the loader, restated
def _double_fold(sd, conv, norm):
    g = sd[norm + ".weight"].astype(np.float64)
    scale = g / np.sqrt(sd[norm + ".running_var"].astype(np.float64) + E.BN_EPS)
    return sd[conv + ".weight"].astype(np.float64) * scale.reshape(-1, 1, 1, 1)


def loaded(sd, conv, norm, dtype, mut=()):
    """(weight, bias) as float64 arrays holding what the kernel holds after
    oamd_net_load_state: the folded fp32 weight (exact_nets.fold) rounded to
    the dtype, the folded fp32 bias. dtype None: nothing is rounded. Mutants:
    w_trunc (weights truncated), w_double (weights rounded from the double
    product, not from its float), bias16 (bias rounded to the dtype),
    head_fp32 (weights left in fp32; the caller passes it for the head convs)."""
    w32, b32 = E.fold(sd, conv, norm)
    w, b = w32.astype(np.float64), b32.astype(np.float64)
    if dtype is None or "head_fp32" in mut:
        return w, b
    p = P_BITS[dtype]
    if "w_double" in mut:
        w = rne(_double_fold(sd, conv, norm), p)
    else:
        w = rne(w, p, "trunc" if "w_trunc" in mut else "rne")
    if "bias16" in mut:
        b = rne(b, p)
    return w, b


# ------------------------------------------------------------------ the tower
@dataclass
class LayerStats:
    name: str
    kinds: tuple            # of "first", "conv1", "conv2", "last"
    unit: float             # every term of the layer's sums is a multiple of it
    bound_units: float      # largest sum of |w||a| + |bias| + |skip|, in units
    max_pre: float          # largest pre-rounding magnitude
    inexact: float          # share of pre-rounding values the dtype does not hold
    ties_down: int          # exact ties resolved toward zero (to even)
    ties_up: int            # ... away from zero (to even)
    neg_inexact: int        # inexact negative values (ReLU sets them to +0 after rounding)
    near_zero: int          # values in (0, one dtype ulp at max_pre]
    neg_near_zero: int      # values in [-half that ulp, 0)
    skip_sensitive: int     # conv2: "add skip, round" != "round, add skip, round"
    live: float             # non-zero share of the stored output


def _layer_kinds(layer: int, nlayers: int) -> tuple:
    k = ["first" if layer == 0 else ("conv1" if layer % 2 == 1 else "conv2")]
    if layer == nlayers - 1:
        k.append("last")
    return tuple(k)


def layer_step(w, b, a, skip, skip_raw, p, mut=(), stats=None, ua=1.0, name="", kinds=()):
    """One conv layer of the spec: y = conv(w, a) + b (+ skip), stored =
    relu(round(y)). Returns (stored, relu(y) unrounded, the output's unit).
    p None: no rounding. stats: a list that receives this layer's LayerStats
    after the exactness conditions were asserted."""
    mode = "trunc" if "trunc" in mut else ("away" if "away" in mut else "rne")
    y0 = conv3x3(w, a) + b[:, None, None]
    y = y0
    if skip is not None:
        sk = skip_raw if "skip_unrounded" in mut else skip
        y = (rne(y0, p, mode) if ("round_before_skip" in mut and p is not None) else y0) + sk
    r = y if p is None else rne(y, p, mode)
    if "relu_late" in mut and p is not None:
        # ReLU before the rounding, done wrong: only values below minus half
        # an ulp (at the layer's largest magnitude) are flushed, smaller
        # negatives survive rounded
        half = 0.5 * ulp_of(max(float(np.abs(y).max()), 1e-30), p)
        stored = np.where(y < -half, 0.0, r)
    else:
        stored = np.maximum(r, 0.0) + 0.0  # -0 -> +0
    unit = ua * E._quantum(w)
    if b.any():
        unit = min(unit, E._quantum(b / unit) * unit)
    # the stored p-bit values are multiples of the ulp at their smallest magnitude
    nz = stored[stored != 0]
    out_unit = unit if (p is None or not nz.size) else max(unit, ulp_of(float(np.abs(nz).min()), p))
    if stats is not None:
        assert p is not None
        # an upper bound of the sum of |w||a| + |bias| + |skip| over every output
        mag = np.abs(w).reshape(w.shape[0], -1).sum(1).max() * np.abs(a).max() + np.abs(b).max()
        if skip is not None:
            mag += np.abs(skip).max()
        bound = float(mag) / unit
        assert bound < E.SUM_BOUND, f"{name}: sum of |terms| = {bound:.3g} units >= 2^24"
        assert np.array_equal(y / unit, np.rint(y / unit)), f"{name}: a value is no multiple of the unit"
        top = float(np.abs(y).max())
        ulp = ulp_of(top, p)
        # the coverage figures are counted over the first COVER_ROWS boards,
        # which every large batch contains: lower bounds for the master batch
        yc, y0c = y[:, :COVER_ROWS], y0[:, :COVER_ROWS]
        inexact, tdown, tup = classify(yc, p)
        sens = 0
        if skip is not None:
            sens = int(np.count_nonzero(rne(yc, p) != rne(rne(y0c, p) + skip[:, :COVER_ROWS], p)))
        stats.append(LayerStats(name, kinds, unit, bound, top, float(inexact.mean()),
                                int(np.count_nonzero(tdown)), int(np.count_nonzero(tup)),
                                int(np.count_nonzero(inexact & (yc < 0))),
                                int(np.count_nonzero((yc > 0) & (yc <= ulp))),
                                int(np.count_nonzero((yc < 0) & (yc >= -0.5 * ulp))), sens,
                                float(np.count_nonzero(stored)) / stored.size))
    return stored, np.maximum(y, 0.0), out_unit


def check_storable(name, v, dtype, pre=None):
    """Every non-zero of v is a normal finite number of the dtype that the
    dtype holds unchanged; fp16: every pre-rounding magnitude <= 2^15."""
    nz = np.abs(v[v != 0])
    if nz.size:
        assert nz.min() >= MIN_NORMAL[dtype] and nz.max() <= MAX_FINITE[dtype], f"{name}: not normal in {dtype}"
    assert representable(v, P_BITS[dtype]), f"{name}: not representable in {dtype}"
    if pre is not None and dtype == "fp16":
        assert pre <= FP16_PRE_MAX, f"{name}: |pre-rounding value| {pre:.6g} > 2^15"


def tower_rounded(sd, x, dtype, mut=(), stats=None, keep=None):
    """The tower of sd on 0/1 planes x (N, cin, 8, 8) under the spec: its
    stored output (C, N, 64) float64 and that output's unit. stats: a list
    that receives every layer's LayerStats (the exactness conditions are
    asserted then); keep: a list that receives every layer's stored output."""
    assert np.isin(x, (0.0, 1.0)).all()
    p = None if dtype is None else P_BITS[dtype]
    a = np.ascontiguousarray(x.transpose(1, 0, 2, 3)).reshape(x.shape[1], x.shape[0], 64).astype(np.float64)
    layers = E.conv_layers(sd)
    ua, raw, skip, skip_raw = 1.0, a, None, None
    for layer, (pc, pn) in enumerate(layers):
        w, b = loaded(sd, pc, pn, dtype, mut)
        if stats is not None:
            check_storable(pc + " weights", w, dtype)
        if layer % 2 == 1:
            skip, skip_raw = a, raw
        second = layer > 0 and layer % 2 == 0
        a, raw, ua = layer_step(w, b, a, skip if second else None, skip_raw, p, mut, stats, ua, pc,
                                _layer_kinds(layer, len(layers)))
        if stats is not None:
            check_storable(pc + " output", a, dtype, stats[-1].max_pre)
        if keep is not None:
            keep.append(a)
    return a, ua


# ------------------------------------------------------------------ the heads
@dataclass
class Reference(E.Reference):
    layers: list = field(default_factory=list)   # LayerStats per conv layer (checked runs)
    head_bound: float = 0.0                      # head convs: largest sum of |terms| in units


def heads_rounded(sd, h, qh, dtype, mut=(), layers=None) -> Reference:
    """The heads of sd on the stored tower output h (C, N, 64) of unit qh:
    dtype-rounded folded 1x1 weights, fp32 accumulator from 0, fp32 bias and
    ReLU, fp32 Linear layers; every sum asserted exact in any order."""
    C, N, _ = h.shape
    hmut = tuple(m for m in mut if m == "head_fp32")
    wp, bp = loaded(sd, "policy_head.conv", "policy_head.norm", dtype, hmut)
    wv, bv = loaded(sd, "value_head.conv", "value_head.norm", dtype, hmut)
    hw = np.concatenate([wp.reshape(2, C), wv.reshape(1, C)])
    hb = np.concatenate([bp, bv])
    X = np.ascontiguousarray(h.reshape(C, N * 64).T)
    live = np.nonzero(np.abs(hw).sum(0))[0]  # the rows read few channels
    asserted = dtype is not None and "head_fp32" not in mut  # else: float64, exactness not claimed
    q, bound = 0.0, 0.0
    if asserted:
        q = E._quantum(hw, hb / qh) * qh
        mag = np.abs(X[:, live]) @ np.abs(hw[:, live]).T + np.abs(hb)
        bound = float(mag.max()) / q
        assert bound < E.SUM_BOUND, f"head convs: sum of |terms| = {bound:.3g} units >= 2^24"
    pre = (X[:, live] @ hw[:, live].T + hb).T.reshape(3, N, 64)
    act = np.maximum(pre, 0.0)
    flat = act[:2].transpose(1, 0, 2).reshape(N, 128)
    exact = E._affine_exact if asserted else (lambda name, W, b, Xx, qx=1.0: (
        Xx @ np.asarray(W, np.float64).T + np.asarray(b, np.float64), 0.0))
    L, step = exact("policy_head.linear", sd["policy_head.linear.weight"], sd["policy_head.linear.bias"], flat, q)
    A, q1 = exact("value_head.linear1", sd["value_head.linear1.weight"], sd["value_head.linear1.bias"], act[2], q)
    z, step_v = exact("value_head.linear2", sd["value_head.linear2.weight"], sd["value_head.linear2.bias"],
                      np.maximum(A, 0.0), q1)
    U = int(min(np.abs(h).max(), 2 ** 31))
    fracs = [s.live for s in layers] if layers else []
    return Reference(L, z[:, 0], U, fracs, step, step_v, list(layers or []), bound)


def forward_rounded(sd, x, dtype, mut=(), check=False, keep=None) -> Reference:
    """The reference: exact arithmetic with the explicit rne() exactly where
    the spec rounds. dtype None switches every rounding off. mut: names from
    MUTANTS, the wrong kernels and loaders of tests/test_cpu_rounding_nets.py.
    check: assert the exactness conditions and collect the LayerStats."""
    assert set(mut) <= set(MUTANTS)
    stats = [] if check else None
    h, qh = tower_rounded(sd, x, dtype, mut, stats, keep)
    return heads_rounded(sd, h, qh, dtype, mut, stats)


def check_scales(ref: E.Reference) -> None:
    """The conditions under which the quarter-step tolerance is meaningful
    (exact_nets.check_scales with this family's spread)."""
    spread = float((ref.logits.max(1) - ref.logits.min(1)).max())
    assert spread <= MAX_SPREAD < 87.0, spread
    assert np.abs(ref.z).max() <= E.MAX_Z
    assert ref.step / 4 >= E.MIN_QUARTER_STEP and ref.step_v / 4 >= E.MIN_QUARTER_STEP, (ref.step, ref.step_v)


# ------------------------------------------------------------------ builders: towers
def _bn_kinds(C):
    """The four exactly folding BatchNorms of exact_nets.integer_tower, by
    channel: (gamma, var, scale), conv bias cb and running mean mu."""
    c = np.arange(C)
    kind = c % 4
    gamma = np.array([1.0, 2.0, 0.5, 1.0])[kind]
    var = np.where((kind == 1) | (kind == 3), E.VAR4, E.VAR1)
    scale = np.array([1.0, 1.0, 0.5, 0.5])[kind]
    cb = 1.0 + c % 2
    mu = cb - 2.0 * ((c // 4) % 3 - 1)
    return gamma, var, scale, cb, mu


def _put_layer(sd, pc, pn, w, bias, C):
    """conv + BatchNorm that fold to exactly (w, bias)."""
    gamma, var, scale, cb, mu = _bn_kinds(C)
    E._put_conv(sd, pc, w / scale[:, None, None, None], cb)
    E._put_bn(sd, pn, bias - (cb - mu) * scale, gamma, mu, var)
    fw, fb = E.fold(sd, pc, pn)
    assert np.array_equal(fw, w) and np.array_equal(fb, bias), f"{pc}: the fold is not the intended one"


TAP_CHOICES = (16, 12, 8, 6, 4, 3, 2, 1)  # +1 taps (and as many -1) per output of a later conv
CAL_ROWS = 128


def rounding_tower(dtype: str, C: int, R: int, cin: int, seed: int = 23):
    """Family R tower and its stored output over the master batch:
    (state dict, h (C, N, 64), unit, LayerStats list). Layer by layer, on the
    reference's own values: the later convs get the most +-1 taps per output
    (TAP_CHOICES) that keep every pre-rounding magnitude below BAND_TOP, and
    every folded bias is -(B + 2 (c mod 3)) with B odd, above 2^p (more
    significant bits than the dtype has) and near the 65th percentile of the
    layer's sums, so a fifth to a third of the outputs stay alive."""
    p = P_BITS[dtype]
    x = E.inputs(cin)
    a = np.ascontiguousarray(x.transpose(1, 0, 2, 3)).reshape(cin, len(x), 64).astype(np.float64)
    sd, stats = {}, []
    names = E.conv_layers({f"residual_blocks.{i}.conv1.weight": 0 for i in range(R)})
    c = np.arange(C)
    ua, raw, skip, skip_raw = 1.0, a, None, None
    for layer, (pc, pn) in enumerate(names):
        ci = cin if layer == 0 else C
        second = layer > 0 and layer % 2 == 0
        if layer % 2 == 1:
            skip, skip_raw = a, raw
        if layer == 0:
            sgn = E._balanced(seed, 100 * C + layer, C, ci * 9, FIRST_TAPS[dtype])
            mag = 1.0 + np.floor(portable_uniform(seed, 200 * C + layer, C * ci * 9).reshape(C, ci * 9)
                                 * FIRST_WMAX[dtype])
            cands = [np.minimum(mag, FIRST_WMAX[dtype]) * sgn]
        else:
            cands = (E._balanced(seed, 100 * C + layer, C, ci * 9, n) for n in TAP_CHOICES)
        for w in cands:  # chosen on the first CAL_ROWS boards with a margin, asserted on all below
            w = w.reshape(C, ci, 3, 3)
            y = conv3x3(w, a[:, :CAL_ROWS])
            if second:
                y += skip[:, :CAL_ROWS]
            B = float(int(max(np.quantile(y, 0.65), 2.0 ** p)) | 1)
            bias = -(B + 2.0 * (c % 3))
            if np.abs(y + bias[:, None, None]).max() <= 0.75 * BAND_TOP[dtype]:
                break
        else:
            raise AssertionError(f"{pc}: no tap count keeps the magnitudes below {BAND_TOP[dtype]}")
        _put_layer(sd, pc, pn, w, bias, C)
        lw, lb = loaded(sd, pc, pn, dtype)
        check_storable(pc + " weights", lw, dtype)
        a, raw, ua = layer_step(lw, lb, a, skip if second else None, skip_raw, p, (), stats, ua, pc,
                                _layer_kinds(layer, len(names)))
        check_storable(pc + " output", a, dtype, stats[-1].max_pre)
        assert stats[-1].max_pre <= BAND_TOP[dtype], f"{pc}: |pre-rounding value| {stats[-1].max_pre} leaves the band"
    return sd, a, ua, stats


def fine_weights(p: int, n: int, phase: int = 0) -> np.ndarray:
    """n weights in [1, 1.25) with p + 3 significant bits, signs mixed: 1 + (8 j
    + k) 2^-(p+2): j the kept low bits (both parities), k the three bits the
    dtype drops, cycling through every pattern with ties (k = 4) at every
    third place; weight 0 carries into the next binade's neighbourhood (all
    kept bits of its field set, rounded up)."""
    i = np.arange(n) + phase
    k = np.where(i % 3 == 0, 4, 1 + (5 * i) % 7)
    j = (3 * i + i // 3) % (1 << (p - 3))
    w = 1.0 + (8.0 * j + k) * 2.0 ** -(p + 2)
    w[0] = 1.0 + (8.0 * ((1 << (p - 3)) - 1) + 6) * 2.0 ** -(p + 2)  # rounds up to 1.25
    return w * np.where((i // 2) % 4 == 3, -1.0, 1.0)


def loader_tower(dtype: str, C: int, R: int, cin: int):
    """Family L tower: exact_nets' routing maps (one (channel, tap) per
    output) with fine_weights as the folded fp32 weights, produced by raw
    weights and the four exactly folding BatchNorms. The first conv's and the
    second convs' weights are positive, the blocks' first convs mix signs."""
    p = P_BITS[dtype]
    sd: dict = {}
    co = np.arange(C)
    maps = [(co % cin, (co + co // cin) % 9)]
    for l in range(R):
        maps += [((5 * co + 3 * l + 1) % C, (co + l) % 9), ((3 * co + 7 * l + 2) % C, (2 * co + l + 4) % 9)]
    names = E.conv_layers({f"residual_blocks.{i}.conv1.weight": 0 for i in range(R)})
    _, var, scale, _, _ = _bn_kinds(C)
    gamma = np.array([1.0, 2.0, 0.5, 1.0])[co % 4]
    for layer, ((pc, pn), (src, tap)) in enumerate(zip(names, maps)):
        ci = cin if layer == 0 else C
        wt = fine_weights(p, C, 5 * layer)
        if layer % 2 == 0:  # a cancelling conv2 would leave tiny sums, whose unit costs the heads their step
            wt = np.abs(wt)
        E._put_conv(sd, pc, E._routing_conv(C, ci, src, tap, wt / scale))
        E._put_bn(sd, pn, np.zeros(C), gamma, None, var)
        fw, _ = E.fold(sd, pc, pn)
        assert np.array_equal(fw[co, src, tap // 3, tap % 3], wt.astype(np.float32)), pc
    return sd


def loader_conditions(sd, dtype) -> dict:
    """What the loader cases must offer, counted over all tower weights:
    folded fp32 weights the dtype does not hold, ties rounding each way, and
    weights whose double product rounds differently than its float."""
    p = P_BITS[dtype]
    out = {"inexact": 0, "ties_down": 0, "ties_up": 0, "double_differs": 0, "trunc_differs": 0}
    for pc, pn in E.conv_layers(sd):
        w32, _ = E.fold(sd, pc, pn)
        w = w32.astype(np.float64)
        nz = w != 0
        inexact, down, up = classify(w[nz], p)
        out["inexact"] += int(inexact.sum())
        out["ties_down"] += int(down.sum())
        out["ties_up"] += int(up.sum())
        out["double_differs"] += int((rne(_double_fold(sd, pc, pn), p) != rne(w, p)).sum())
        out["trunc_differs"] += int((rne(w, p, "trunc") != rne(w, p)).sum())
    return out


# ------------------------------------------------------------------ builders: heads
def add_sparse_heads(sd: dict, h: np.ndarray, qh: float, hid: int, dtype: str, rot: int = 0,
                     fine: bool = False) -> dict:
    """Heads for a tower whose stored output over the master batch is h
    (C, N, 64) of unit qh. Row r of the head convs (0, 1 policy, 2 value)
    reads the K channels (rot + 5 (3 i + r)) mod C with weights +1, -1
    alternating (fine: fine_weights, which the dtype does not hold; the fine
    value row reads 4 channels with positive weights and is thresholded at 1,
    just below every single weight); the policy rows' ReLU thresholds sit at
    the median. Policy Linear: logit a <
    64 is square a of channel 0 minus square (11 a + 3) mod 64 of channel 1,
    logit 64 square 17 of channel 0 minus square 40 of channel 1, plus small
    biases, x 2^-k for a spread of at most MAX_SPREAD; K is the largest of
    32 .. 1 for which the logits' step keeps 4 x MIN_QUARTER_STEP. Value:
    hidden unit j = ReLU(window - v[(5 j + 1) mod 64]) of the thresholded value
    conv output v, summed with weights +1, -1 alternating, x 2^-k for |z| <=
    MAX_Z; the window is the widest power of two (in units) that keeps the
    step."""
    C, N, _ = h.shape
    p = P_BITS[dtype]
    X = h.reshape(C, N * 64)
    need = 4 * E.MIN_QUARTER_STEP

    def rows_of(K):
        hw = np.zeros((3, C))
        for r in range(3):
            # fine value row: 4 channels, so that many squares hold exactly one
            # live weight, which the window above the threshold 1 resolves
            k = min(K, 4) if (fine and r == 2) else K
            ch = (rot + 5 * (3 * np.arange(k) + r)) % C
            hw[r, ch] = np.abs(fine_weights(p, k, 7 * r)) if (fine and r == 2) else (
                fine_weights(p, k, 7 * r) if fine else np.where(np.arange(k) % 2 == 0, 1.0, -1.0))
        return hw

    for K in (32, 16, 8, 4, 2, 1):
        hw = rows_of(K)
        hwq = rne(hw, p)  # what the kernel multiplies with
        q = E._quantum(hwq) * qh
        pre = (hwq @ X).reshape(3, N, 64)
        theta = np.floor(np.array([np.quantile(pre[0], 0.5), np.quantile(pre[1], 0.5)]) / q) * q
        act = np.maximum(pre[:2] - theta[:, None, None], 0.0)
        T = np.zeros((65, 128))
        a = np.arange(64)
        T[a, a] = 1.0
        T[a, 64 + (11 * a + 3) % 64] = -1.0
        T[64, 17], T[64, 64 + 40] = 1.0, -1.0
        flat = act.transpose(1, 0, 2).reshape(N, 128)
        L0 = flat @ T.T
        tq = 2.0 ** np.floor(np.log2(max(float(np.abs(L0).max()), q) / 16.0))
        t = ((7 * np.arange(65)) % 5 - 2.0) * max(tq, q)
        L = L0 + t
        s = E._pow2_scale(float((L.max(1) - L.min(1)).max()), MAX_SPREAD)
        if q * s >= need or K == 1:
            break
    E._put_conv(sd, "policy_head.conv", hw[:2].reshape(2, C, 1, 1))
    E._put_bn(sd, "policy_head.norm", -theta)
    sd["policy_head.linear.weight"] = (T * s).astype(np.float32)
    sd["policy_head.linear.bias"] = (t * s).astype(np.float32)
    # value: threshold at the median of the positive sums (fine: at 1, just
    # below every single weight), then the window
    pv = pre[2]
    tv = 1.0 if fine else np.floor(np.quantile(pv, 0.5) / q) * q
    v = np.maximum(pv - tv, 0.0)
    j = np.arange(hid)
    W1 = np.zeros((hid, 64))
    W1[j, (5 * j + 1) % 64] = -1.0
    w2 = np.where(j % 2 == 0, 1.0, -1.0)
    for k in range(16, -1, -1):
        win = q * 2.0 ** k
        H = np.maximum(win - v[:, (5 * j + 1) % 64], 0.0)
        zr = H @ w2
        b2 = -np.round(np.median(zr) / q) * q
        sv = E._pow2_scale(float(np.abs(zr + b2).max()), E.MAX_Z)
        if q * sv >= need:
            break
    else:
        raise AssertionError("value head: no window keeps the step")
    E._put_conv(sd, "value_head.conv", hw[2:].reshape(1, C, 1, 1))
    E._put_bn(sd, "value_head.norm", np.array([-tv]))
    sd["value_head.linear1.weight"] = W1.astype(np.float32)
    sd["value_head.linear1.bias"] = np.full(hid, win, np.float32)
    sd["value_head.linear2.weight"] = (w2 * sv).reshape(1, hid).astype(np.float32)
    sd["value_head.linear2.bias"] = np.array([b2 * sv], np.float32)
    return sd


# ------------------------------------------------------------------ cases
def coverage_failures(ref: Reference, dtype: str) -> list:
    """The coverage conditions of the tower nets, per conv layer: the list of
    those not met (empty = all met)."""
    bad = []
    for s in ref.layers:
        want = {"inexact share": s.inexact >= COVER_INEXACT, "ties down": s.ties_down >= COVER_MIN,
                "ties up": s.ties_up >= COVER_MIN, "negative inexact": s.neg_inexact >= COVER_MIN,
                "within one ulp above zero": s.near_zero >= COVER_MIN,
                "within half an ulp below zero": s.neg_near_zero >= COVER_MIN}
        if "conv2" in s.kinds:
            want["skip-order sensitive"] = s.skip_sensitive >= COVER_MIN
        bad += [f"{s.name} ({'/'.join(s.kinds)}): {k}" for k, ok in want.items() if not ok]
    return bad


@functools.lru_cache(maxsize=None)
def case(dtype: str, family: str, C: int, R: int, cin: int = 17, hid: int = 64):
    """(state dict, master inputs, Reference over the master batch) of one
    net; a batch of n rows is inputs[:n] against reference.rows(n). The
    exactness conditions are asserted here, for the tower nets the coverage
    conditions too."""
    x = E.inputs(cin)
    rot = 7 * R + hid % 5 + (3 if dtype == "fp16" else 0)
    if family == "R":
        tower, h, qh, stats = rounding_tower(dtype, C, R, cin)
    else:
        tower = loader_tower(dtype, C, R, cin) if family == "L" else E.routing_tower(C, R, cin, 0)
        stats = []
        h, qh = tower_rounded(tower, x, dtype, (), stats)
    sd = add_sparse_heads(dict(tower), h, qh, hid, dtype, rot, fine=family == "H")
    ref = heads_rounded(sd, h, qh, dtype, (), stats)
    check_scales(ref)
    if family == "R":
        bad = coverage_failures(ref, dtype)
        assert not bad, f"{case_id((dtype, family, C, R, cin, hid))}: coverage conditions not met: {bad}"
    return sd, x, ref


def case_id(args) -> str:
    dtype, family, C, R, cin, hid = args
    return f"{dtype}-{family}-c{C}b{R}-in{cin}-hid{hid}"


# What tests/test_gpu_resnet_rounding.py runs: (case arguments, row counts).
# 1 and 5 (3 at C=256) rows: one board per workgroup; 1024 / 1027 (1025): the
# throughput geometries with a ragged last workgroup.
DTYPES = ("bf16", "fp16")
ROWS = {128: (1, 5, 1024, 1027), 256: (3, 1025)}
TOWER = [((dt, "R", C, R, 17, 64), ROWS[C]) for dt in DTYPES
         for C, R in ((128, 0), (128, 1), (128, 2), (256, 1), (256, 2))]
TOWER += [((dt, "R", 128, 1, 17, 33), (5, 1027)) for dt in DTYPES]
TWO_ROWS = {128: (5, 1027), 256: (3, 1025)}
LOADER = [((dt, "L", C, R, 17, 64), TWO_ROWS[C]) for dt in DTYPES for C, R in ((128, 0), (128, 1), (256, 1))]
HEADCONV = [((dt, "H", C, 0, 17, 64), TWO_ROWS[C]) for dt in DTYPES for C in (128, 256)]
ALL_CASES = TOWER + LOADER + HEADCONV


# ------------------------------------------------------------------ wide-range heads
# exact_nets keeps the logit spread at most 16 and |z| at most 3. Two head
# variants on one exact tower (exact logits in either dtype) leave that range.
WIDE_SPREAD = (64.0, 80.0)   # every probability still a normal fp32 number (spread < 87)
WIDE_OFFSET = 200.0          # the logits' absolute size: needs the max subtraction
WIDE_Z = 9.0
# Policy criterion, derived: relative error of a probability at most
# 2^-23 (|o - m| + 8). __expf(d) is exp2 of the fp32 product d log2e: the
# product's rounding and the constant's contribute at most 1.5 x 2^-24 |d|; a
# few ulps (8 x 2^-23 allows 8) come from exp2, the sum and the reciprocal.
WIDE_REL = 2.0 ** -23
WIDE_ULPS = 8.0
WIDE_TOWER = ("A", 128, 1, 17, 0)


@functools.lru_cache(maxsize=None)
def wide_heads_case(which: str):
    """(state dict, master inputs, exact_nets.Reference) of the exact routing
    net 128x1b with one head rescaled. "policy": the 65 logits x m 2^k (m odd,
    so the sums stay exact) for a largest spread of 64-80, all offset by +200,
    and logit 64 shifted so that it is the row's maximum (the kernel's o64
    path) in about half the rows and a square is in the others. "value": the
    value pre-activation x the small integer that brings max |z| into (6, 9]."""
    sd, x, ref0 = E.case("A", 128, 1, 17, 64, 0)
    _, (h, U, fracs) = E._tower(*WIDE_TOWER)
    sd = dict(sd)
    if which == "policy":
        W = sd["policy_head.linear.weight"].astype(np.float64)
        b = sd["policy_head.linear.bias"].astype(np.float64)
        L = ref0.logits
        shift = np.round(np.median(L[:, :64].max(1) - L[:, 64]) / ref0.step) * ref0.step
        L = L + shift * (np.arange(65) == 64)
        spread = float((L.max(1) - L.min(1)).max())
        f = next(c for c in sorted(m * 2.0 ** k for m in range(1, 16, 2) for k in range(8))
                 if WIDE_SPREAD[0] <= c * spread <= WIDE_SPREAD[1])
        b = (b + shift * (np.arange(65) == 64)) * f + WIDE_OFFSET
        sd["policy_head.linear.weight"] = (W * f).astype(np.float32)
        sd["policy_head.linear.bias"] = b.astype(np.float32)
        assert np.array_equal(sd["policy_head.linear.weight"], W * f)
        assert np.array_equal(sd["policy_head.linear.bias"], b)
    else:
        assert which == "value"
        zmax = float(np.abs(ref0.z).max())
        f = next(float(m) for m in range(2, 64) if 2.0 * WIDE_Z / 3.0 < m * zmax <= WIDE_Z)
        for k in ("value_head.linear2.weight", "value_head.linear2.bias"):
            v = sd[k].astype(np.float64) * f
            sd[k] = v.astype(np.float32)
            assert np.array_equal(sd[k], v)
    ref = E.heads_exact(sd, h, U, fracs)  # asserts the 2^24 bounds of the rescaled sums
    if which == "policy":
        spread = float((ref.logits.max(1) - ref.logits.min(1)).max())
        assert WIDE_SPREAD[0] <= spread <= WIDE_SPREAD[1] < 87.0, spread
        on64 = float((ref.logits.argmax(1) == 64).mean())
        assert 0.1 <= on64 <= 0.9 and ref.logits.min() > 100.0, on64
    else:
        assert 2.0 * WIDE_Z / 3.0 < np.abs(ref.z).max() <= WIDE_Z
    return sd, x, ref


def wide_outputs(ref: E.Reference):
    """float64 softmax and tanh of the exact logits and z."""
    d = ref.logits - ref.logits.max(1, keepdims=True)
    e = np.exp(d)
    return e / e.sum(1, keepdims=True), np.tanh(ref.z), d


def wide_deviations(policy, value, ref: E.Reference) -> dict:
    """The wide-range criteria's figures: the largest relative error of a
    probability and the largest in units of its bound 2^-23 (|o - m| + 8),
    |sum p - 1|, and the largest |dvalue| (bound exact_nets.MIN_QUARTER_STEP)."""
    p64, v64, d = wide_outputs(ref)
    rel = np.abs(np.asarray(policy, np.float64) - p64) / p64
    bound = WIDE_REL * (np.abs(d) + WIDE_ULPS)
    return {"rel": float(rel.max()), "rel_over_bound": float((rel / bound).max()),
            "bound_at_worst": float(bound.flat[int((rel / bound).argmax())]),
            "sum_err": float(np.abs(np.asarray(policy, np.float64).sum(1) - 1.0).max()),
            "value_err": float(np.abs(np.asarray(value, np.float64) - v64).max())}
