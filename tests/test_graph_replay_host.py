"""The case table of tests/test_gpu_graph_replay.py, checked on the CPU: what the GPU file claims to drive the kernels
through must follow from the table itself, before any GPU run.

A replay's tick offset is the number of steps the handle has taken since the capture.  The kernels derive from the counter
their alignment inside a four-tick Philox block and the head of a delay line kept in memory, so the offsets of a case must
visit every residue mod 4 and, with a delay, more than one residue mod the delay -- one of them not zero."""
import os

import pytest

import graph_replay_cases as cases


def test_the_offsets_of_the_issue_example():
    c = dict(K=32, between=(1, 2, 3, 5))
    assert cases.offsets(c) == [0, 33, 67, 102, 139]
    for d in (2, 3, 4):
        res = {o % d for o in cases.offsets(c)}
        assert len(res) >= 2 and res != {0}, (d, res)
    assert {o % 4 for o in cases.offsets(c)} == {0, 1, 2, 3}


@pytest.mark.parametrize("name", sorted(cases.CASES) + ["by_value"])
def test_offsets_hit_every_block_residue_and_move_the_ring_head(name):
    c = cases.BY_VALUE_CASE if name == "by_value" else cases.CASES[name]
    offs = cases.offsets(c)
    assert len(offs) == cases.REPLAYS == 5 and offs[0] == 0
    assert all(b >= 1 for b in c["between"])
    assert {o % 4 for o in offs} == {0, 1, 2, 3}, (name, offs)
    d = cases.delay_of(c)
    if d > 0:
        res = {o % d for o in offs}
        assert len(res) >= 2 and any(r != 0 for r in res), (name, d, offs)


def test_every_family_has_a_case_on_each_rng_mode_it_serves():
    seen = {}
    for name, c in cases.CASES.items():
        assert c["family"] in cases.FAMILIES, name
        seen.setdefault(c["family"], set()).add(c["rng"])
    for fam, both in cases.FAMILIES.items():
        assert "philox" in seen.get(fam, ()), fam
        if both:
            assert seen[fam] == {"numpy", "philox"}, (fam, seen[fam])


def test_cases_are_well_formed():
    for name, c in cases.CASES.items():
        assert c["N"] in (256, 320), name                   # one full block, or one full and one ragged
        assert c["K"] > 1, name                             # fused launches: K = 1 is step_graph's
        assert c["call"] in ("rollout",) + cases.CLOSED_CALLS, name
        closed = c["call"] in cases.CLOSED_CALLS
        assert closed == (c["family"] in ("policy", "learn", "learn_pe", "eval", "summary", "nlev")), name
        assert (c["learner"] is not None) == (closed and c["call"] != "policy"), name
        assert c["mutate"] in (None, "policy", "rates", "levels"), name
        assert ("PHILOX=%d" % (c["rng"] == "philox") in c["has"]) or c["family"] == "image", name
        if c["levels"]:
            assert all(k in c["config"] for k in cases.NLEV_CREATED), name
        if c["mutate"] == "levels":
            assert c["levels"] and len(set(cases.NLEV_TN)) == len(set(cases.NLEV_TN2)), name
    # the dispatch thresholds: lean at K >= 32, quiet at K >= 16
    assert all(c["K"] >= 32 for c in cases.CASES.values() if c["family"] == "lean")
    assert all(c["K"] >= 16 for c in cases.CASES.values() if c["family"] == "quiet")
    assert min(c["K"] for c in cases.CASES.values() if c["family"] == "lean") == 32
    assert min(c["K"] for c in cases.CASES.values() if c["family"] == "quiet") == 16
    # one ragged case per family that allows it
    for fam in ("lean", "quiet", "general", "cline", "cstep", "grid", "policy", "learn", "learn_pe", "eval", "summary", "nlev"):
        assert any(c["N"] == 320 for c in cases.CASES.values() if c["family"] == fam), fam
    # several launches per captured call
    sp = [c for c in cases.CASES.values() if "LEARN_SHORT_PIECES" in c["opts"]]
    assert sp and all(c["K"] == 12 for c in sp)              # pieces of at most 5 steps: three launches
    # the image pipeline forks to the side stream from two batches on (batches of 64 steps for a handle of this size)
    assert any(c["family"] == "image" and c["K"] > 64 for c in cases.CASES.values())


def test_level_arrays_keep_the_number_of_levels():
    tn, rn = cases.level_arrays(320)
    tn2, rn2 = cases.level_arrays(320, cases.NLEV_TN2, cases.NLEV_RN2)
    assert len(set(tn)) == len(set(tn2)) == 5 and (tn != tn2).any() and (rn != rn2).any()
    assert 0.0 in tn and 0.0 in tn2                          # a level without a draw on both sides
    a, e = cases.pe_arrays(320, 1)
    assert a.dtype == e.dtype == "float32" and (a > 0).all() and (a <= 1).all() and (e >= 0).all() and (e <= 1).all()


def test_only_the_listed_cases_are_insensitive_to_the_offset():
    """Withholding the offset at a replay must break every case but the few numpy-stream ones without a delay line in memory
    (run once on the GPU while the cases were written: exactly these passed, every other case failed its comparison)."""
    assert sorted(n for n, c in cases.CASES.items() if not cases.needs_offset(c)) == sorted(cases.BY_VALUE_WOULD_DO)
    assert cases.needs_offset(cases.BY_VALUE_CASE)


def test_no_allocation_on_the_closed_loop_launch_paths():
    """A launch entry point may be under a graph capture: the translation units and headers of the closed-loop launchers
    allocate, free and synchronise nothing (the setters in mdpp_capi.hip do)."""
    csrc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mdp_playground_amd", "csrc")
    files = [f for f in sorted(os.listdir(csrc))
             if f.startswith(("mdpp_discrete_closed", "mdpp_discrete_policy", "mdpp_discrete_learn", "mdpp_discrete_eval")) and f.endswith((".hip", ".hpp"))]
    assert len(files) >= 20, files
    for f in files:
        with open(os.path.join(csrc, f)) as fh:
            text = fh.read()
        for word in ("hipMalloc", "hipFree", "hipMemcpy", "hipMemset", "Synchronize"):
            assert word not in text, (f, word)
