"""The host half of the K/V-cache family answers what it answered when tests/golden/kvcache_host_answers.json was recorded: every _plan, _workspace and
_suggest_splits entry point, tfa_kvcache_varlen_schedule_size and tfa_kvcache_varlen_schedule_plan, over the fixture's grid of calls (both dtypes, head dims, GQA
groups, row counts, capacities contiguous and paged, chunk counts, packing modes, 16-bit and e4m3 caches, packed q plain and scheduled, windows, trees, and the
refusals one by one) — status, (grid, block, lds), workspace words and chunk counts, row by row.  No GPU: plans never launch."""
import importlib.util
import json
import os

import pytest

from tiny_flash_attention_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_kvcache_host_answers", os.path.join(GOLDEN, "make_kvcache_host_answers.py"))
GEN = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(GEN)

ERR_STRIDE = -5


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "kvcache_host_answers.json")) as f:
        d = json.load(f)
    assert tuple(d["entry_points"]) == GEN.ENTRY_POINTS
    return d["cases"]


def test_every_recorded_row_is_answered_as_recorded(recorded):
    L = _lib.lib()
    assert len(recorded) * len(GEN.ENTRY_POINTS) >= 3000      # (a few thousand rows: 375 cases x 20 entry points)
    wrong = []
    for row in recorded:
        got = GEN.answers(L, row["case"])
        assert len(got) == len(row["answers"]) == len(GEN.ENTRY_POINTS)
        wrong += [(row["case"], name, want, have) for name, want, have in zip(GEN.ENTRY_POINTS, row["answers"], got) if want != have]
    assert not wrong, f"{len(wrong)} rows differ, the first: {wrong[:5]}"


def test_the_fixture_covers_what_it_is_there_for(recorded):
    cases = [dict(GEN.DEFAULTS, **r["case"]) for r in recorded]
    seen = lambda k: {tuple(c[k]) if isinstance(c[k], list) else c[k] for c in cases}  # noqa: E731
    assert seen("dtype") >= {_lib.TFA_BF16, _lib.TFA_F16} and seen("D") >= {64, 72, 128, 256}
    assert {(c["H"], c["Hk"]) for c in cases} >= {(8, 8), (8, 2), (8, 1), (256, 1)} and seen("Nq") >= {1, 5, 33, 130}
    assert {(c["cap"], c["page"]) for c in cases} >= {(n, pg) for n in (1024, 16384, 65536) for pg in (0, 128)}
    assert seen("splits") >= {1, 3, 64, 1000} and seen("pack") >= {0, 1, 2, 7} and seen("causal") == {0, 1} and seen("fp8") == {0, 1}
    assert seen("vq") >= {None, (1, 3), (5, 9), (130, 200), (5, 3)} and seen("left") >= {-1, 0, 63, 1023, 1 << 30}
    assert seen("sched") == {0, 1} and seen("tree") == {0, 1, 2}
    muts = {m for c in cases for m in c["mut"]}
    for ptr in GEN.POINTERS:
        assert {"null:" + ptr, "misalign:" + ptr} <= muts
    assert {"reserved", "reserved2", "vq_reserved", "group_past_2gib", "out_noncontig", "k_new"} <= muts
    assert any(c["H"] % c["Hk"] for c in cases if c["Hk"])
    # every entry point both answers and refuses somewhere in the grid
    for i, name in enumerate(GEN.ENTRY_POINTS):
        col = [r["answers"][i] for r in recorded]
        if name.endswith("suggest_splits"):
            assert min(col) == 1 and max(col) > 1, name
        else:
            status = [a[0] if isinstance(a, list) else min(a, 0) for a in col]
            assert 0 in status and min(status) < 0, name


def test_a_group_past_2gib_runs_unpacked_or_is_refused_when_scheduled(recorded):
    """4-D: packing is an optimisation — the plan is the unpacked one; scheduled: the list was built for the packing named — TFA_ERR_STRIDE, never a silent change."""
    ix = {n: i for i, n in enumerate(GEN.ENTRY_POINTS)}
    by_case = {json.dumps(r["case"], sort_keys=True): r["answers"] for r in recorded}
    hit4 = hits = 0
    for r in recorded:
        c = r["case"]
        if c.get("mut") != ["group_past_2gib"] or c.get("pack") != 1:
            continue
        if "vq" not in c and c.get("Nq", 5) == 5:
            off = by_case[json.dumps(dict(c, pack=2), sort_keys=True)]
            for name in ("pack_plan", "window_plan", "tree_plan"):
                assert r["answers"][ix[name]] == off[ix[name]] and r["answers"][ix[name]][0] == 0, (c, name)
            hit4 += 1
        if c.get("sched"):
            assert r["answers"][ix["sched_plan"]][0] == ERR_STRIDE and r["answers"][ix["window_plan"]][0] == ERR_STRIDE and r["answers"][ix["tree_plan"]][0] == ERR_STRIDE
            hits += 1
    assert hit4 and hits
