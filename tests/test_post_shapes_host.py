"""tests/post_shape_cases.py without a GPU: the table reaches every kernel form tests/test_gpu_post_shapes.py is meant
to reach (by the table's own pure-Python statement of the forms), and the oracle those GPU tests compare against is
pinned at every new shape: its pictures against a numpy restatement of get_transformed_image
(gym_env_wrapper.py:523-618) at every geometry of the table, its flush on done against np.sum at the delays around
numpy's pairwise blocks."""
import numpy as np
import pytest

import post_shape_cases as cases
from oracle import oracle as ora


@pytest.mark.parametrize("name", sorted(cases.PICTURE))
def test_picture_case_gets_the_form_it_is_listed_for(name):
    p = cases.PICTURE[name]
    hw, ch, pad = p["hw"], p["ch"], cases.pic_pad(p)
    th = hw + 2 * pad
    assert cases.image_form(hw, ch, pad) == (p["form"], p["lds"], p["per_cu"])
    assert (th * th * ch) % 4 == 0 and hw % 2 == 0                   # mdpp_post_create takes it
    assert p["tr"] != "shift" or pad >= 1
    src, dst, tags = cases.source_dwords(p), cases.canvas_dwords(p), p["tags"]
    if p["form"] == cases.LDS:
        assert ("over48k" in tags) == (p["lds"] > 48 * 1024)
    for tier in (2, 4, 6):
        if "tier%d" % tier in tags:
            assert p["per_cu"] == tier
    if "multipass" in tags:             # both loops of k_post_image_lds run more than once ...
        assert p["form"] == cases.LDS and src > cases.PASS_DWORDS and dst > cases.PASS_DWORDS
    if "ragged_pass" in tags:           # ... and end on a pass that only some lanes take part in
        assert "multipass" in tags and src % cases.PASS_DWORDS and dst % cases.PASS_DWORDS
    if "largest_lds" in tags:
        assert cases.lds_bytes(hw, ch) <= cases.LDS_LIMIT < cases.lds_bytes(hw + 2, ch)
    if "past_lds_limit" in tags:        # refused for its LDS alone
        assert cases.lds_bytes(hw, ch) > cases.LDS_LIMIT and (hw * ch) % 4 == 0 and (th * ch) % 4 == 0 and ch <= 16
    if "ragged_canvas_row" in tags:
        assert (th * ch) % 4 != 0 and (hw * ch) % 4 == 0 and ch <= 16
    if "c_over_16" in tags:
        assert ch > 16 and (hw * ch) % 4 == 0 and (th * ch) % 4 == 0
    if "c16" in tags:
        assert ch == 16
    if "smallest_lds" in tags:
        assert (hw, src) == (2, 2)
    if "smallest_general" in tags:
        assert (hw, ch) == (2, 1)
    if "no_draw" in tags:
        assert "shift" not in p["tr"]
    if "quant_over_pad" in tags:
        assert p["shq"] > pad
    if "one" in tags:
        assert (p["N"], p["K"]) == (1, 1)
    if "lds_wrap" in tags:              # more pictures in a fused call than workgroups in the grid
        assert p["form"] == cases.LDS and p["N"] * p["K"] > cases.NUM_CUS * p["per_cu"] >= p["N"]
    if "general_wrap" in tags:
        assert p["form"] == cases.GEN and cases.general_blocks(p, p["N"] * p["K"]) > cases.GENERAL_MAX_BLOCKS
        assert p["N"] * p["K"] >= 3100
    else:
        assert p["form"] == cases.LDS or cases.general_blocks(p, p["N"] * p["K"]) <= cases.GENERAL_MAX_BLOCKS


def test_table_reaches_every_form():
    tags = set().union(*(p["tags"] for p in cases.PICTURES))
    assert tags >= {"tier6", "tier4", "tier2", "over48k", "largest_lds", "past_lds_limit", "ragged_canvas_row", "multipass", "ragged_pass",
                    "funnel", "c16", "c_over_16", "smallest_lds", "smallest_general", "no_draw", "quant_over_pad", "one",
                    "lds_wrap", "general_wrap"}
    by = {(p["hw"], p["ch"], cases.pic_pad(p)): p for p in cases.PICTURES}
    for geo in ((84, 3, 20), (84, 1, 20), (100, 3, 20), (120, 3, 4), (128, 3, 2), (140, 3, 2), (144, 3, 2), (84, 3, 1),
                (2, 2, 1), (2, 1, 1), (6, 2, 1), (32, 4, 3), (8, 16, 2), (8, 17, 2), (12, 3, 0)):
        assert geo in by, geo
    assert "philox" in cases.PICTURE["84x84x3_pad20_q4"]["rngs"]
    # both picture kernels wrap, the LDS form at 16 x 16 x 3 and past 48 KiB; both get a single picture and a masked reset
    wraps = [p for p in cases.PICTURES if "lds_wrap" in p["tags"]]
    assert {(p["hw"], "over48k" in p["tags"]) for p in wraps} == {(16, False), (128, True)}
    assert {p["form"] for p in cases.PICTURES if "one" in p["tags"]} == {cases.LDS, cases.GEN}
    assert {cases.PICTURE[n]["form"] for n in cases.MASKED_RESET} == {cases.LDS, cases.GEN}
    assert all(cases.PICTURE[n]["hw"] == 84 for n in cases.MASKED_RESET)
    assert {(p["N"], p["K"]) for p in cases.PICTURES} >= {(1, 1), (65, 3), (257, 3)}
    assert all(p["delay"] >= 1 for p in cases.PICTURES)
    # the step kernel: every ring form, the register ring at both ends and at numpy's first pairwise block, the cap
    assert cases.RING_DELAYS == [0, 1, 7, 8, 9, 16, 17, 128] and cases.REFUSED_DELAY == cases.MAX_DELAY + 1
    assert [cases.step_form(d) for d in cases.RING_DELAYS] == [(0, 0), (2, 1), (2, 7), (2, 8), (1, 0), (1, 0), (0, 0), (0, 0)]
    assert cases.RING_CALLS == [7, 8, 17] and cases.RING_N == 257
    # K: below, at and above the prefetch depth, its multiples (empty tail) and their neighbours
    assert cases.K_SEQUENCE == [1, cases.PRE - 1, cases.PRE, cases.PRE + 1, 2 * cases.PRE - 1, 2 * cases.PRE, 2 * cases.PRE + 1]
    assert sorted(cases.step_form(d)[0] for d in cases.K_SEQUENCE_DELAYS) == [0, 2]
    assert sorted(cases.step_form(d)[0] for d in cases.NO_AUTORESET_DELAYS) == [0, 1, 2]
    assert cases.N_CASES == [1, 63, 64, 65, 255, 256, 257, 1000]
    assert cases.CONT_DIMS == [1, 3, 17] and cases.CONT_NOISES == [0.2, 0.0, None]
    assert cases.ACTION_COUNTS == [2, 6, 64, 300] and cases.ACTION_NOISES == [0.0, 0.25, 1.0]
    assert cases.FLUSH_DELAYS == [7, 8, 9, 16, 17, 127, 128]
    assert cases.kernel_name("philox", 3, (84, 3, 20)) == "k_post_step<PHILOX=1,RING=2,DC=3> + k_post_image_lds<LDS=21840,PER_CU=6>"
    assert cases.kernel_name("numpy", 40, (84, 3, 1)) == "k_post_step<PHILOX=0,RING=0,DC=0> + k_post_image"


GEOMETRIES = sorted({(p["hw"], p["ch"], cases.pic_pad(p), p["tr"], p["shq"] or 1) for p in cases.PICTURES})


@pytest.mark.parametrize("hw,ch,pad,tr,shq", GEOMETRIES)
def test_oracle_picture_equals_numpy_restatement(hw, ch, pad, tr, shq):
    """Pixels and end stream of PostOracle.reset / .step against draw, truncate, paste, transpose in numpy."""
    r = np.random.default_rng(hw * 1000 + ch * 10 + pad)
    for seed in range(6):
        gen = np.random.default_rng(seed + 7)
        o = ora.PostOracle("discrete", n_actions=4, image_shape=(hw, hw, ch), image_transforms=tr, image_padding=pad,
                           image_sh_quant=shq)
        o.set_rng(ora.pcg_words(gen))
        for t in range(3):
            img = r.integers(0, 256, size=(hw, hw, ch)).astype(np.uint8)
            want = cases.np_picture(gen, img, pad, "shift" in tr, shq)
            got = o.reset(img) if t == 0 else o.step(img, 0.0, False)[0]
            assert got.shape == want.shape == (hw + 2 * pad, hw + 2 * pad, ch)
            assert np.array_equal(got, want), (seed, t)
        assert np.array_equal(o.get_rng(), ora.pcg_words(gen)), seed


def test_funnel_case_places_pictures_at_every_byte_offset():
    """top * C mod 4 decides the byte funnel's shift in k_post_image_lds: the first canvases of the `funnel` case (as the
    GPU test seeds them) see 1, 2 and 3; the reference-golden geometry with image_sh_quant 4 sees 0 only."""
    for name, want in (("84x84x3_pad20_q1", {0, 1, 2, 3}), ("84x84x3_pad20_q4", {0})):
        p = cases.PICTURE[name]
        seen = set()
        for i in range(p["N"]):
            top, _ = cases.np_place(cases.wrapper_generator(cases.SEED + cases.ENV0 + i), p["hw"], cases.pic_pad(p), True, p["shq"] or 1)
            seen.add((top * p["ch"]) & 3)
        assert seen == want, (name, seen)


@pytest.mark.parametrize("delay", cases.FLUSH_DELAYS)
def test_oracle_flush_is_numpy_sum(delay):
    """A done step pays reward + np.sum(buffer * scale + shift) + term * scale, then noise-free scale and shift
    (gym_env_wrapper.py:407-432), on rewards whose sums round: the order of the additions shows."""
    r = np.random.default_rng(delay)
    scale, shift, term = -2.0, 0.25, 1.5
    for trial in range(20):
        o = ora.PostOracle("discrete", n_actions=2, delay=delay, reward_scale=scale, reward_shift=shift, term_state_reward=term)
        o.reset()
        pushed = r.normal(size=delay) * 10.0 ** r.integers(-3, 4, size=delay)
        for x in pushed:
            assert o.step(None, x, False)[1] == 0.0 * scale + shift
        assert np.array_equal(o.ring(), pushed)
        last = float(r.normal())
        want = last
        want += np.sum(np.asarray(list(pushed), dtype=np.float64) * scale + shift)
        want += term * scale
        want += 0.0
        want *= scale
        want += shift
        got = o.step(None, last, True)[1]
        assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64), (delay, trial)
        assert np.array_equal(o.ring(), pushed)                # a done step neither pushes nor pops
        o.clear_ring()
        assert not o.ring().any()


def test_oracle_counters_setter_leaves_the_action_counter_alone():
    """set_philox puts action_tick at tick; set_counters sets the three apart -- what a batch needs after a masked reset
    moved its reset counter for every instance."""
    kw = dict(n_actions=6, transition_noise=0.25, delay=2)
    a, b = ora.PostOracle("discrete", **kw), ora.PostOracle("discrete", **kw)
    a.set_philox(5, 9)
    b.set_philox(5, 9)
    seq = [a.action(3) for _ in range(40)]
    b.set_counters(0, 0, 17)
    assert [b.action(3) for _ in range(23)] == seq[17:]
    assert len(set(seq)) > 1
