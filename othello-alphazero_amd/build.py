"""Build the MI355X-native othello_mcts extension in-tree.

  liboamd.so               HIP kernels (tree.hip, selfplay.hip, arena.hip, positions.hip over the headers wave.h,
                           tree_search.h, tree_game.h; resnet.hip, replay.hip, solver.hip, adjudicate.hip, exact_leaves.hip,
                           baseline.hip)
                           + the C ABI
                           (capi.hip and, by subsystem, capi_net.hip, capi_play.hip, capi_data.hip; capi_version.hip
                           carries the source hashes), hipcc --offload-arch=gfx950
  _othello_mcts_impl*.so   pybind11 host layer (pybind_module.cpp) over the C ABI

Both land in othello-alphazero_amd/othello_mcts/ (git-ignored, shipped to the
GPU box with the snapshot). Usage: python othello-alphazero_amd/build.py [-j N]
"""

from __future__ import annotations

import argparse
import concurrent.futures as cf
import os
import subprocess
import sys
import sysconfig
from pathlib import Path

HERE = Path(__file__).resolve().parent
CSRC = HERE / "csrc"
PKG = HERE / "othello_mcts"
INCLUDE = HERE.parent / "include"
BUILD = HERE / "build"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = os.environ.get("OAMD_ARCH", "gfx950")

COMMON = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-I", str(CSRC), "-I", str(INCLUDE),
          "-Wall", "-Wno-unused-function", "-fno-gpu-rdc", *os.environ.get("OAMD_EXTRA_FLAGS", "").split()]
# the tree units (TREE_UNITS) / rng.h, capi.hip's tables and capi_net.hip's weight fold must
# reproduce the reference's float arithmetic bit for bit: no FMA contraction,
# IEEE division and sqrt. The C ABI's other host units share inline host code
# with those two (capi_internal.h), so they are built the same way.
EXACT = ["-ffp-contract=off", "-fno-fast-math"]
# the tree kernels read statistics, links and game state that the same wave
# has just written with vector stores (ordered by a wavefront fence, wave.h
# wave_order): no global load may go through the scalar cache, which does not
# see those stores (tests/test_cpu_host.py checks the ISA)
NO_SCALAR_LOADS = ["-mllvm", "-amdgpu-scalarize-global-loads=false"]
# every unit that includes tree_search.h or tree_game.h is built this way
TREE_UNITS = ("tree.hip", "selfplay.hip", "arena.hip", "positions.hip")
UNITS = {
    **{u: EXACT + NO_SCALAR_LOADS for u in TREE_UNITS},
    "capi.hip": EXACT,
    "capi_net.hip": EXACT,
    "capi_play.hip": EXACT,
    "capi_data.hip": EXACT,
    "capi_version.hip": [],
    # packed replay buffer: its value targets are SampleBuffer's, bit for bit
    "replay.hip": EXACT,
    # accumulators and fragments in arch VGPRs: the default heuristic parks the
    # 128 accumulators of a 1-wave/SIMD tile in AGPRs and shuffles them per MFMA;
    # the max-ILP machine scheduler: k_resnet_w8 0.895-0.900 vs 0.907-0.913 ms per
    # 4096 rows (3 same-box pairs, outputs bit-identical; tools/ab_run1.sh)
    "resnet.hip": os.environ.get("OAMD_RESNET_FLAGS",
                                 "-mllvm -amdgpu-mfma-vgpr-form=1 -mllvm -amdgpu-sched-strategy=max-ilp").split()
    + ["-Rpass-analysis=kernel-resource-usage"],
    # exact endgame solver: integer code; its searcher stacks are LDS, and the
    # build fails if a search kernel (k_solve, k_solve_items) reports any
    # scratch (check_solver_scratch)
    "solver.hip": ["-Rpass-analysis=kernel-resource-usage"],
    # adjudication's apply kernel: integer code
    "adjudicate.hip": [],
    # exact leaf values: the solver's integer code on a 10-level
    # LDS stack; the build fails if a solve kernel reports any scratch
    "exact_leaves.hip": ["-Rpass-analysis=kernel-resource-usage"],
    # baseline opponents: integer search on a 10-level LDS
    # stack, the pick's one float product as rng.h needs it; the build fails if
    # k_baseline reports any scratch
    "baseline.hip": EXACT + ["-Rpass-analysis=kernel-resource-usage"],
}


# k_resnet_w8 (8 waves, 2 per SIMD) must allocate <= 208 VGPRs per wave so one
# k_select wave (93 VGPRs) still fits beside it on each SIMD (resnet.hip)
W8_VGPR_LIMIT = 208
# k_resnet_w4 (4 waves, 1 per SIMD): VGPRs + AGPRs of the SIMD's 512 unified
# registers; 4 x 0 + 416 + the 96 of a k_tree wave = 512. No scratch: a spill
# inside the tower would put memory traffic between its MFMAs.
W4_VGPR_LIMIT = 416


def run(cmd: list[str]) -> None:
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(" ".join(cmd) + "\n" + r.stdout + r.stderr)
        raise SystemExit(f"build failed: {cmd[-1]}")
    if "kernel-resource-usage" in " ".join(cmd):
        # the remarks of a unit are checked by that unit's rule only
        checks = {**RESOURCE_CHECKS, **SCRATCH_CHECKS}
        unit = next((u for u in checks if str(CSRC / u) in cmd), None)
        if unit:
            checks[unit](r.stderr)
    elif r.stderr.strip():
        sys.stderr.write(r.stderr)


def kernel_remarks(remarks: str):
    """(kernel name, field, value) of -Rpass-analysis=kernel-resource-usage remarks."""
    name = None
    for ln in remarks.splitlines():
        if "Function Name:" in ln:
            name = ln.split("Function Name:")[1].split()[0]
        elif name and "remark:" in ln and ":" in ln.split("remark:")[1]:
            field, _, value = ln.split("remark:")[1].split("[-Rpass")[0].rpartition(":")
            yield name, field.strip(), value.strip()


def check_solver_scratch(remarks: str) -> None:
    """solver.hip: the searcher stacks of k_solve and of the split solver's
    item kernel k_solve_items live in LDS; a runtime-indexed per-thread array
    would land in scratch. Fail if either search kernel reports any (the
    planning and reducing kernels hold no stack and are not checked)."""
    seen = 0
    for name, field, value in kernel_remarks(remarks):
        search = "k_solve" in name and "reduce" not in name and "plan" not in name
        if search and field.startswith("ScratchSize"):
            seen += 1
            if int(value.split()[0]) != 0:
                raise SystemExit(f"build failed: {name} uses {value} bytes of scratch per lane: "
                                 "the solver's stacks must stay in LDS")
    if not seen:
        raise SystemExit("build failed: no resource remark for k_solve in solver.hip")


def check_w8_vgprs(remarks: str) -> None:
    """Parse -Rpass-analysis=kernel-resource-usage remarks; fail if a k_resnet_w8
    instantiation's VGPR allocation (granule 8) exceeds W8_VGPR_LIMIT."""
    name = None
    seen = 0
    for ln in remarks.splitlines():
        if "Function Name:" in ln:
            name = ln.split("Function Name:")[1].split()[0]
        elif name and "k_resnet_w8" in name and " VGPRs:" in ln:
            v = int(ln.split("VGPRs:")[1].split()[0])
            seen += 1
            if (v + 7) // 8 * 8 > W8_VGPR_LIMIT and os.environ.get("OAMD_W8_VGPR_CHECK", "1") != "0":
                raise SystemExit(f"build failed: {name} uses {v} VGPRs (> {W8_VGPR_LIMIT}): "
                                 "k_select could no longer co-reside with the ResNet kernel")
    if not seen:  # A/B builds with other geometries (e.g. -DOAMD_WC=128) have no w8 kernel
        sys.stderr.write("note: no k_resnet_w8 kernel in this build\n")


def check_w4_resources(remarks: str) -> None:
    """k_resnet_w4 (not its extra-round loop kernel, which runs nearly empty
    launches): VGPRs + AGPRs (granule 8) <= W4_VGPR_LIMIT and no scratch."""
    regs: dict[str, int] = {}
    for name, field, value in kernel_remarks(remarks):
        if "k_resnet_w4" not in name or "k_resnet_w4_loop" in name:
            continue
        if field in ("VGPRs", "AGPRs"):
            regs[name] = regs.get(name, 0) + (int(value.split()[0]) + 7) // 8 * 8
        elif field.startswith("ScratchSize") and int(value.split()[0]) != 0:
            raise SystemExit(f"build failed: {name} uses {value} bytes of scratch per lane")
    for name, v in regs.items():
        if v > W4_VGPR_LIMIT:
            raise SystemExit(f"build failed: {name} uses {v} VGPRs + AGPRs (> {W4_VGPR_LIMIT}): "
                             "a k_tree wave could no longer co-reside with the ResNet kernel")
    if not regs:
        raise SystemExit("build failed: no resource remark for k_resnet_w4 in resnet.hip")


def check_resnet(remarks: str) -> None:
    check_w8_vgprs(remarks)
    check_w4_resources(remarks)


def check_exact_leaves_scratch(remarks: str) -> None:
    """exact_leaves.hip: k_solve_leaves and k_solve_positions keep their
    searcher stacks in LDS (17,920 bytes per wave); fail on any scratch."""
    seen = 0
    for name, field, value in kernel_remarks(remarks):
        if "k_solve" in name and field.startswith("ScratchSize"):
            seen += 1
            if int(value.split()[0]) != 0:
                raise SystemExit(f"build failed: {name} uses {value} bytes of scratch per lane: "
                                 "the exact-leaf solver's stack must stay in LDS")
    if not seen:
        raise SystemExit("build failed: no resource remark for k_solve_leaves in exact_leaves.hip")


def check_baseline_scratch(remarks: str) -> None:
    """baseline.hip: k_baseline keeps its searcher stack in LDS (20,480 bytes
    per wave); fail on any scratch (k_baseline_pick holds no stack and is not
    checked)."""
    seen = 0
    for name, field, value in kernel_remarks(remarks):
        if "k_baseline" in name and "pick" not in name and field.startswith("ScratchSize"):
            seen += 1
            if int(value.split()[0]) != 0:
                raise SystemExit(f"build failed: {name} uses {value} bytes of scratch per lane: "
                                 "the baseline search's stack must stay in LDS")
    if not seen:
        raise SystemExit("build failed: no resource remark for k_baseline in baseline.hip")


RESOURCE_CHECKS = {"resnet.hip": check_resnet, "solver.hip": check_solver_scratch}
# units whose every search kernel must stay without scratch (its stack is LDS)
SCRATCH_CHECKS = {"exact_leaves.hip": check_exact_leaves_scratch, "baseline.hip": check_baseline_scratch}


def newer(out: Path, deps: list[Path]) -> bool:
    return out.exists() and all(out.stat().st_mtime >= d.stat().st_mtime for d in deps)


def source_hash_defines() -> list[str]:
    """-D flags carrying the source hashes (othello_mcts/provenance.py) into
    capi_version.hip, so the library reports what it was built from."""
    sys.path.insert(0, str(PKG))
    try:
        import provenance
    finally:
        sys.path.pop(0)
    return [f'-DOAMD_SOURCE_HASH_{k.upper()}="{provenance.source_hash(k)}"' for k in provenance.FAMILIES]


def build(jobs: int = 4, force: bool = False) -> None:
    BUILD.mkdir(exist_ok=True)
    headers = list(CSRC.glob("*.h")) + [INCLUDE / "othello_mcts_amd.h", INCLUDE / "othello_mcts_amd_experimental.h"]
    hashes = source_hash_defines()
    objs = []
    todo = []
    all_srcs = [CSRC / u for u in UNITS] + headers
    for unit, extra in UNITS.items():
        src = CSRC / unit
        obj = BUILD / (unit + ".o")
        objs.append(obj)
        # the version unit carries the hashes of every source: rebuilt when any changes
        versioned = unit == "capi_version.hip"
        deps = all_srcs if versioned else [src, *headers]
        if force or not newer(obj, [*deps, Path(__file__)]):
            todo.append([HIPCC, *COMMON, *extra, *(hashes if versioned else []), "-c", str(src),
                         "-o", str(obj)])
    with cf.ThreadPoolExecutor(max_workers=max(1, jobs)) as ex:
        list(ex.map(run, todo))
    lib = PKG / "liboamd.so"
    if force or todo or not lib.exists():
        run([HIPCC, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", str(lib), *map(str, objs)])

    # pybind11 host layer: plain C++ against the C ABI, no torch headers
    import pybind11

    ext = sysconfig.get_config_var("EXT_SUFFIX")
    mod = PKG / f"_othello_mcts_impl{ext}"
    src = CSRC / "pybind_module.cpp"
    if force or not newer(mod, [src, *headers, lib, Path(__file__)]):
        run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-fvisibility=hidden",
             "-I", pybind11.get_include(), "-I", sysconfig.get_paths()["include"], "-I", str(INCLUDE),
             str(src), "-o", str(mod), "-L", str(PKG), "-loamd", "-Wl,-rpath,$ORIGIN"])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", "--jobs", type=int, default=4)
    ap.add_argument("--force", action="store_true")
    a = ap.parse_args()
    build(a.jobs, a.force)
    print("built", *sorted(p.name for p in PKG.glob("*.so")))
