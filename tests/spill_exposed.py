"""The kernels of the default-flag translation units that spill SGPRs AND VGPRs -- the SGPR-into-VGPR-lane spill hazard
of docs/round6.md section 10 -- and the GPU case that covers each one.

By default the compiler parks spilled SGPRs in the lanes of a VGPR; where that VGPR is itself spilled to scratch inside
divergent control flow, only the active lanes are stored and the values parked in the inactive lanes are lost.  The
translation units in SPILL_SAFE_UNITS are built with SPILL_SAFE (build.py: SGPRs spill to memory).  Every other unit
keeps the compiler's default, and a kernel of such a unit with sgpr_spill_count > 0 and vgpr_spill_count > 0 in its
code-object metadata is EXPOSED (a conservative rule: the metadata does not say which VGPR was spilled where).  It is not
a complete one: built without SPILL_SAFE, the round-6 kernel itself, k_continuous_step<DMAX=32, OMAX=4, PHILOX>, reports
4 746 SGPR spills and 3 040 B of scratch but a vgpr_spill_count of 0 (its scratch is the state vectors), so the rule
would not flag it; that unit is covered by the pinned SPILL_SAFE_UNITS instead.

tests/test_kernel_spills.py reads the built objects and fails unless the exposed set equals EXPOSED's keys;
tests/test_gpu_spill_lanes.py runs each entry's case on every lane against the oracle, with resets that diverge
inside waves.  Keys are (kernel, template arguments) as parsed from the mangled name by parse_mangled; for
k_continuous_rollout_fast the arguments are <D, ORDER, NREL, NOISE, HELPER, GEN, PHILOX, NPROD, K1, PAR, Z0T>."""
import re

# the units build.py must compile with SPILL_SAFE (pinned here, checked against build.EXTRA_FLAGS and the command stamps)
SPILL_SAFE_UNITS = ("mdpp_continuous.hip", "mdpp_continuous_line8.hip", "mdpp_discrete.hip", "mdpp_discrete_wide.hip",
                    "mdpp_discrete_long.hip", "mdpp_discrete_quiet.hip", "mdpp_discrete_quiet_nu.hip")
SPILL_SAFE_FLAG = "-amdgpu-spill-sgpr-to-vgpr=0"

CFAST_PARAMS = ("D", "ORDER", "NREL", "NOISE", "HELPER", "GEN", "PHILOX", "NPROD", "K1", "PAR", "Z0T")
_LIT = re.compile(r"L[a-z](n?)(\d+)E")


def parse_mangled(sym):
    """'_ZN4mdpp25k_continuous_rollout_fastILi12ELi2E...EEv...' -> ('k_continuous_rollout_fast', (12, 2, ...)): a kernel of
    namespace mdpp and its template arguments when all of them are integer / bool literals (None where one is not)."""
    m = re.match(r"_ZN4mdpp(\d+)", sym)
    if not m:
        return sym, None
    n = int(m.group(1))
    p = m.end()
    name = sym[p:p + n]
    p += n
    if sym[p:p + 1] != "I":
        return name, ()
    p += 1
    args = []
    while True:
        lm = _LIT.match(sym, p)
        if not lm:
            break
        args.append(-int(lm.group(2)) if lm.group(1) else int(lm.group(2)))
        p = lm.end()
    return name, (tuple(args) if sym[p:p + 1] == "E" else None)


def parse_dispatched(name):
    """A formatted kernel name of env.rollout_kernel_name(K) -> the same key as parse_mangled gives for the kernel launched:
    'k_continuous_rollout_fast<D=12,...,NPROD=2>' (HELPER=1 forms) and 'k_continuous_step1<...,PAR=1>' (K1 = true, the
    rollout kernel's one-step instantiation with HELPER = false and NPROD = 1)."""
    m = re.fullmatch(r"(k_continuous_rollout_fast|k_continuous_step1)<(.*)>", name)
    assert m, name
    kv = dict(x.split("=") for x in m.group(2).split(","))
    v = {k: int(x) for k, x in kv.items()}
    if m.group(1) == "k_continuous_step1":
        assert v.get("PAR") == 1, name     # (the WG= forms are launched with PAR = false)
        t = dict(v, HELPER=0, NPROD=1, K1=1, PAR=1, Z0T=0)
    else:
        assert v["HELPER"] == 1 and v["NOISE"] == 1, name     # (HELPER=0 prints NPROD=0 for a launched NPROD of 1)
        t = dict(v, K1=0, PAR=0, Z0T=v.get("Z0", 0))
    return "k_continuous_rollout_fast", tuple(t[k] for k in CFAST_PARAMS)


def describe(key):
    name, args = key
    if name == "k_continuous_rollout_fast" and args is not None:
        return name + "<" + ",".join(f"{k}={a}" for k, a in zip(CFAST_PARAMS, args)) + ">"
    return f"{name}<{args}>"


def _cf(D, ORDER, NREL, GEN, PHILOX, NPROD):
    """a rollout kernel with transition / reward noise and helper waves"""
    return "k_continuous_rollout_fast", (D, ORDER, NREL, 1, 1, GEN, PHILOX, NPROD, 0, 0, 0)


def _k1par(D, ORDER, NREL, GEN):
    """the one-step kernel with the step's normals made side by side (numpy streams, transition noise)"""
    return "k_continuous_rollout_fast", (D, ORDER, NREL, 1, 0, GEN, 0, 1, 1, 1, 0)


# (unit, scratch bytes, SGPR / VGPR spill counts at the commit that wrote this table, in the comment)
EXPOSED = {
    # mdpp_continuous_fast.o: the rollout kernels with transition / reward noise and helper waves
    _cf(8, 2, 4, 0, 0, 2): "r8o2n4_np2",               # 92 B scratch, 38 SGPR / 22 VGPR spills
    _cf(8, 2, 4, 0, 1, 2): "r8o2n4_px2",               # 60 B, 30 / 14
    _cf(8, 2, 4, 1, 1, 2): "r8o2n4_px2_gen",           # 76 B, 205 / 18
    _cf(8, 2, 8, 0, 0, 2): "r8o2n8_np2",               # 92 B, 42 / 22
    _cf(8, 2, 8, 0, 1, 2): "r8o2n8_px2",               # 60 B, 31 / 14
    _cf(8, 2, 8, 1, 0, 2): "r8o2n8_np2_gen",           # 128 B, 309 / 25
    _cf(8, 2, 8, 1, 1, 2): "r8o2n8_px2_gen",           # 48 B, 285 / 6
    _cf(12, 1, 4, 0, 0, 2): "r12o1n4_np2",             # 92 B, 49 / 22
    _cf(12, 1, 4, 0, 1, 2): "r12o1n4_px2",             # 84 B, 60 / 20
    _cf(12, 1, 4, 1, 1, 2): "r12o1n4_px2_gen",         # 196 B, 215 / 48
    _cf(12, 1, 12, 0, 0, 2): "r12o1n12_np2",           # 92 B, 57 / 22
    _cf(12, 1, 12, 0, 1, 2): "r12o1n12_px2",           # 84 B, 70 / 20
    _cf(12, 1, 12, 1, 0, 2): "r12o1n12_np2_gen",       # 204 B, 388 / 50
    _cf(12, 1, 12, 1, 1, 2): "r12o1n12_px2_gen",       # 204 B, 346 / 50
    _cf(12, 2, 4, 0, 0, 1): "r12o2n4_np1",             # 76 B, 18 / 18
    _cf(12, 2, 4, 0, 0, 2): "r12o2n4_np2",             # 420 B, 38 / 104 (BASELINE cfg5's rollout kernel)
    _cf(12, 2, 4, 0, 1, 1): "r12o2n4_px1",             # 68 B, 34 / 16
    _cf(12, 2, 4, 0, 1, 2): "r12o2n4_px2",             # 420 B, 36 / 104
    _cf(12, 2, 4, 1, 0, 1): "r12o2n4_np1_gen",         # 80 B, 246 / 9
    _cf(12, 2, 4, 1, 0, 2): "r12o2n4_np2_gen",         # 64 B, 195 / 4
    _cf(12, 2, 4, 1, 1, 2): "r12o2n4_px2_gen",         # 352 B, 186 / 77
    _cf(12, 2, 12, 0, 0, 1): "r12o2n12_np1",           # 76 B, 22 / 18
    _cf(12, 2, 12, 0, 0, 2): "r12o2n12_np2",           # 420 B, 42 / 104
    _cf(12, 2, 12, 0, 1, 1): "r12o2n12_px1",           # 68 B, 54 / 16
    _cf(12, 2, 12, 0, 1, 2): "r12o2n12_px2",           # 436 B, 50 / 104
    _cf(12, 2, 12, 1, 0, 1): "r12o2n12_np1_gen",       # 96 B, 390 / 12
    _cf(12, 2, 12, 1, 0, 2): "r12o2n12_np2_gen",       # 448 B, 380 / 99
    _cf(12, 2, 12, 1, 1, 1): "r12o2n12_px1_gen",       # 48 B, 336 / 2
    _cf(12, 2, 12, 1, 1, 2): "r12o2n12_px2_gen",       # 368 B, 336 / 81
    # mdpp_continuous_step1.o: the one-step kernels (PAR)
    _k1par(12, 2, 4, 0): "s12o2n4_par",                # 20 B, 10 / 4 (BASELINE cfg5's one-step kernel)
    _k1par(12, 2, 12, 0): "s12o2n12_par",              # 32 B, 10 / 7
    _k1par(12, 2, 12, 1): "s12o2n12_par_gen",          # 2960 B, 20 / 46
}


def divergent_steps(ends, single, wave=64):
    """Per wave of `wave` envs: the number of steps on which SOME but not all of its lanes ended an episode (and so ran the
    in-step reset while the others did not) -- the trigger of the hazard.  `ends`: _check_vs_oracle's `flags` list of (K, [K, N]
    terminated | truncated); only the calls of the kind checked count (single: the one-step launches, K = 1)."""
    per_wave = None
    for K, f in ends:
        if (K == 1) != single:
            continue
        n = f.reshape(K, -1, wave).sum(axis=2)
        d = ((n > 0) & (n < wave)).sum(axis=0)
        per_wave = d if per_wave is None else per_wave + d
    return per_wave


def assert_resets_diverge(ends, single, min_steps=8):
    """Every wave sees at least `min_steps` steps with divergent resets."""
    per_wave = divergent_steps(ends, single)
    assert per_wave is not None and len(per_wave) and per_wave.min() >= min_steps, None if per_wave is None else per_wave.tolist()
    return per_wave
