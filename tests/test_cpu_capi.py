"""The foreign host's view of the C ABI (tests/capi_host.py), without a GPU.

A host written against include/othello_mcts_amd.h has to reproduce five
structures and the prototypes it calls; nothing else pinned them. Here:
  * a C probe compiled from the header prints sizeof and every field's
    offsetof, which must equal the ctypes classes', field by field;
  * every function capi_host binds is exported and declared under that name;
  * INTEGRATION.md §3's SearchConfig block names the same fields and types;
  * the two whole-game configurations of tests/test_gpu_capi.py's sparse-host
    test do reach, on the reference alone, the events that test is about
    (threads with no batch waiting, terminal leaves inside a waiting batch).
"""

import ctypes
import re
import subprocess

import numpy as np
import pytest

import asym_stub as A
import capi_host as H
import oracle as O
from conftest import ROOT

HEADER_TEXT = H.HEADER.read_text()


def _strip_comments(text: str) -> str:
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def header_struct_fields(name: str) -> list:
    """Field names of `typedef struct NAME { ... } NAME;` in declaration order."""
    m = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), _strip_comments(HEADER_TEXT), re.S)
    assert m, name
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if decl:
            fields.append(re.search(r"(\w+)\s*$", decl).group(1))
    return fields


# --------------------------------------------------------------------- layout
@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    """{struct: (sizeof, {field: offsetof})} as a C compiler lays the header out."""
    d = tmp_path_factory.mktemp("capi_layout")
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "othello_mcts_amd.h"', "int main(void) {"]
    for name in H.STRUCTS:
        lines.append(f'    printf("{name} sizeof %zu\\n", sizeof({name}));')
        for f in header_struct_fields(name):
            lines.append(f'    printf("{name} {f} %zu\\n", offsetof({name}, {f}));')
    lines += ["    return 0;", "}", ""]
    (d / "probe.c").write_text("\n".join(lines))
    # compiled as C: the product header promises a plain-C surface
    subprocess.run(["g++", "-x", "c", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(d / "probe.c"),
                    "-o", str(d / "probe")], check=True)
    out = subprocess.run([str(d / "probe")], check=True, capture_output=True, text=True).stdout
    layout: dict = {}
    for line in out.splitlines():
        name, field, value = line.split()
        size, offsets = layout.get(name, (None, {}))
        if field == "sizeof":
            size = int(value)
        else:
            offsets[field] = int(value)
        layout[name] = (size, offsets)
    return layout


@pytest.mark.parametrize("name", list(H.STRUCTS))
def test_ctypes_structures_have_the_headers_layout(c_layout, name):
    cls = H.STRUCTS[name]
    size, offsets = c_layout[name]
    assert [f[0] for f in cls._fields_] == header_struct_fields(name) == list(offsets)
    assert ctypes.sizeof(cls) == size
    for field, _ in cls._fields_:
        assert getattr(cls, field).offset == offsets[field], (name, field)
    # every field is as wide as the gap to the next one: no field of another width fits the same offsets
    ends = sorted(offsets.values())[1:] + [size]
    for (field, _), end in zip(cls._fields_, ends):
        assert getattr(cls, field).offset + getattr(cls, field).size == end, (name, field)


def test_position_is_40_bytes(c_layout):
    assert c_layout["oamd_position"][0] == 40 == ctypes.sizeof(H.Position)
    assert c_layout["oamd_root_info"][0] == 64 == ctypes.sizeof(H.RootInfo)
    assert np.dtype(H.Position).itemsize == 40


# ----------------------------------------------------------------- prototypes
def test_bound_functions_are_exported_and_declared():
    declared = set(re.findall(r"\b(oamd_[a-z0-9_]+)\s*\(", _strip_comments(HEADER_TEXT)))
    raw = ctypes.CDLL(str(H.LIB_PATH))
    for name, (res, args) in H.PROTOTYPES.items():
        assert name in declared, name
        assert hasattr(raw, name), name
        assert res is not None and all(a is not None for a in args), name
    bound = H.lib()
    for name, (res, args) in H.PROTOTYPES.items():
        fn = getattr(bound, name)
        assert list(fn.argtypes) == list(args), name
        assert fn.restype is (ctypes.c_int if res == H.STATUS else res), name
    # the step API, the root queries and the net are all there
    for name in ("oamd_engine_search_begin", "oamd_engine_select", "oamd_engine_leaf_flags", "oamd_engine_features",
                 "oamd_engine_set_evaluation", "oamd_engine_backup", "oamd_engine_status", "oamd_engine_set_stream",
                 "oamd_net_forward", "oamd_engine_search"):
        assert name in H.PROTOTYPES


def test_abi_version_is_the_headers():
    version = int(re.search(r"#define\s+OAMD_ABI_VERSION\s+(\d+)", HEADER_TEXT).group(1))
    assert H.lib().oamd_abi_version() == version


def test_prototype_arity_matches_the_header():
    """Each bound prototype has as many arguments as the header's declaration."""
    text = _strip_comments(HEADER_TEXT)
    for name, (_, args) in H.PROTOTYPES.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        params = m.group(1).strip()
        n = 0 if params in ("", "void") else params.count(",") + 1
        assert n == len(args), (name, params)


def test_status_codes_map_to_the_reference_exceptions():
    """OAMD_INVALID_ARGUMENT -> ValueError, OAMD_OUT_OF_RANGE
    -> IndexError, with oamd_last_error()'s message (argument checks that never
    reach the device)."""
    for code, name in enumerate(("OAMD_OK", "OAMD_INVALID_ARGUMENT", "OAMD_OUT_OF_RANGE", "OAMD_RUNTIME",
                                 "OAMD_CAPACITY")):
        assert int(re.search(r"\b%s\s*=\s*(\d+)" % name, HEADER_TEXT).group(1)) == code == getattr(H, name)
    L = H.lib()
    with pytest.raises(ValueError, match="n must be >= 0"):
        L.oamd_get_legal_moves(None, None, None, -1, None)
    cfg = H.SearchConfig(4, 64, 1, 8, 20000.0, 2.5, 0.0, 0.5)
    handle = ctypes.c_void_p()
    with pytest.raises(ValueError, match="num_games must be >= 1"):
        L.oamd_engine_create(0, 0, 0, ctypes.byref(cfg), 1, ctypes.byref(handle))
    p = H.Position()
    L.oamd_initial_position(ctypes.byref(p))
    assert p.tuple() == O.initial_position().tuple()


# -------------------------------------------------------------- documentation
def integration_python_block() -> str:
    text = (ROOT / "INTEGRATION.md").read_text()
    section = text[text.index("## 3. "):]
    section = section[:section.index("\n## 4. ")]
    return re.search(r"```python\n(.*?)```", section, re.S).group(1)


def test_integration_md_search_config_is_the_hosts():
    block = integration_python_block()
    m = re.search(r"class SearchConfig\(ctypes\.Structure\):\s*_fields_\s*=\s*\[(.*?)\]", block, re.S)
    assert m
    documented = re.findall(r'\(\s*"(\w+)"\s*,\s*ctypes\.(\w+)\s*\)', m.group(1))
    assert len(documented) == len(H.SearchConfig._fields_) == m.group(1).count("(")
    for (name, ctype), (want_name, want_type) in zip(documented, H.SearchConfig._fields_):
        assert name == want_name
        assert getattr(ctypes, ctype) is want_type, name


def test_integration_md_block_is_an_excerpt_of_the_host():
    """Every statement of the documented binding stands in tests/capi_host.py
    (whitespace aside), so the document cannot drift from the executed form."""
    def squeeze(s):
        return re.sub(r"\s+", "", s)

    host = squeeze((ROOT / "tests" / "capi_host.py").read_text())
    block = integration_python_block()
    chunks = [c for c in re.split(r"\n\s*\n", block) if c.strip()]
    assert len(chunks) >= 3
    for chunk in chunks:
        code = "\n".join(line for line in chunk.splitlines() if not line.lstrip().startswith("#"))
        assert squeeze(code) in host, chunk


# ----------------------------------------------------------- input conditions
@pytest.mark.parametrize("name", list(H.WHOLE_GAMES))
def test_whole_game_configurations_reach_the_sparse_events_on_the_oracle(name):
    """The reference alone, games g = 0..2 of engine seed 17 with the asymmetric
    stub, greedy, until the first game ends: per game at least 3 searches in
    which fewer than T * steps batches went to the NN (a thread had no batch
    waiting, or its batch was all terminal) and at least 10 NN calls holding an
    all-zero row (a terminal leaf inside a waiting batch). Without them the
    sparse-host test of tests/test_gpu_capi.py would pass vacuously."""
    cfg = H.WHOLE_GAMES[name]
    G = H.WHOLE_GAME_GAMES
    full = cfg["num_threads"] * H.search_steps(cfg)
    taps = [H.EvaluatorTap(A.asymmetric_stub) for _ in range(G)]
    refs = [O.OracleMCTS(game_key=A.game_key(H.WHOLE_GAME_SEED, g), **cfg) for g in range(G)]
    skipped, zero_rows, moves = [0] * G, [0] * G, 0
    while all(r.position().player != 0 for r in refs):
        for g, (r, tap) in enumerate(zip(refs, taps)):
            tap.clear()
            r.search(tap)
            assert len(tap.calls) <= full
            skipped[g] += len(tap.calls) < full
            zero_rows[g] += tap.zero_row_calls()
            a = O.legal_actions(r.position())[int(np.argmax(r.visit_counts()))]
            r.apply_action(a)
        moves += 1
    print(f"configuration {name}: moves={moves} searches with skipped NN calls={skipped} "
          f"NN calls with an all-zero row={zero_rows}")
    assert moves >= 30
    assert min(skipped) >= H.SKIPPED_SEARCHES_FLOOR, skipped
    assert min(zero_rows) >= H.ZERO_ROW_CALLS_FLOOR, zero_rows
