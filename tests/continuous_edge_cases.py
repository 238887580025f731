"""Continuous envs at the edges of float32: the case table, the action scripts and the trajectory driver shared by
tests/test_continuous_edges_host.py (CPU: C oracle against the numpy restatement, coverage of every edge) and
tests/test_gpu_continuous_edges.py (every kernel form against the oracle).  numpy only; nothing of the product is imported.

What the uniform(-1.2, 1.2) actions of the other continuous tests never produce, and what the scripts here produce on
purpose:
  * a coordinate exactly on +-state_space_max, reached with a clip and without one (Box.contains is inclusive);
  * an action exactly on +-action_space_max, and one ulp outside it;
  * a distance exactly equal to target_radius (the reference tests `<`), a state on the face of a terminal hypercube;
  * -0.0, subnormal, NaN and +-inf actions; on unbounded action boxes also actions whose square overflows float32;
  * the unbounded boxes (state_space_max / action_space_max left at their default, inf).

A script is a float32 [T, N, D] action array.  Every env's script starts with a wall run -- +action_space_max in every
dimension for as many steps as the dynamics need to cross the box from rest -- followed by a body of palette values, moves
that walk off the wall and back, pushes into the wall and plain uniform actions.  Lanes 0-63 share one script (whole waves
then hold only admitted, or only rejected, actions); every other lane runs a rotation of the body with uniform draws of its
own (mixed waves).  T = 96 is cut into launches of 64, 1 and 31 steps.
"""
import numpy as np

F32 = np.float32
T = 96
LAUNCHES = (64, 1, 31)          # the single step goes through step(): the one-step kernel forms
FLT_MAX = float(np.finfo(F32).max)
FLT_MIN = float(np.finfo(F32).tiny)                                  # 2^-126
DENORM_MIN = float(np.nextafter(F32(0), F32(1)))                     # 1.4e-45
DENORM_MAX = float(np.nextafter(F32(FLT_MIN), F32(0)))               # the largest subnormal
INF, NAN = float("inf"), float("nan")
U = None                        # a script slot filled with a uniform draw


def _base(D, **kw):
    cfg = dict(state_space_type="continuous", state_space_dim=D, reward_function="move_to_a_point",
               transition_dynamics_order=1, inertia=1.0, time_unit=1.0, make_denser=True, seed=31)
    cfg.update(kw)
    return cfg


# coverage: the least number of events PER ENV ON AVERAGE over the host test's envs; 3 wherever the case admits the
# event at all.  The exceptions are argued where they are set.
_COMMON = dict(rejected=3, truncations=3)

CASES = {}


def _case(name, config, *, max_episode_steps=24, autoreset=("same_step",), rngs=("numpy",), Ns=(300,), rollout=(), step=(),
          coverage=None, body="point", line=False, wall=0):
    cov = dict(_COMMON)
    cov.update(coverage or {})
    CASES[name] = dict(config=config, max_episode_steps=max_episode_steps, autoreset=autoreset, rngs=rngs, Ns=Ns,
                       rollout=rollout, step=step, coverage=cov, body=body, line=line, wall=wall)


# States on the integer lattice: the wall run ends on (4, 4); (3, 4) is at distance exactly 5.0 = target_radius (not
# inside: `<`), (4, 3) is a corner of the terminal cube [-3, 4] x [-4, 3] (terminal: Box.contains is inclusive), and
# 3 -> 4 lands on the wall without a clip.  Everything within the radius ends the episode, so an env lives on (4, 4) and
# (3, 4) only.  The two cubes (edge 7) cover all of the box but 2.6 of its 64 units of area, and reset() resamples out of
# them (25 draws per reset on average): 58 % of the resets land where (+1, +1) twice leads to (4, 4), the others end in
# the circle or a cube at once.  max_episode_steps = 40 fits twice into 96 steps: one truncation per env is asked for.
_case("o1_lattice",
      _base(2, state_space_max=4, action_space_max=1, target_point=[0, 0], target_radius=5.0, make_denser=False,
            reward_scale=2.0, reward_shift=-0.25, term_state_reward=0.5, terminal_states=[[0.5, -0.5], [-1.0, 0.6]],
            term_state_edge=7.0),
      max_episode_steps=40, autoreset=("same_step", "next_step"), body="lattice", wall=16,
      rollout=("k_continuous_rollout_fast<D=2,ORDER=1,NREL=2,NOISE=0,HELPER=0,GEN=1,",),
      step=("k_continuous_step1<D=2,ORDER=1,NREL=2,NOISE=0,GEN=1,",),
      coverage=dict(clips=3, on_wall_unclipped=3, at_radius=3, cube_face=3, truncations=1))

# inertia 3 is no power of two (the IEEE-division branch); the action penalty is always computed
_case("o2_inertia3",
      _base(2, transition_dynamics_order=2, inertia=3.0, time_unit=0.1, state_space_max=0.0625, action_space_max=1,
            target_point=[0.01, -0.02], target_radius=0.004, action_loss_weight=0.01),
      rollout=("k_continuous_rollout_fast<D=2,ORDER=2,NREL=2,NOISE=0,HELPER=0,GEN=0,",),
      step=("k_continuous_step1<D=2,ORDER=2,NREL=2,NOISE=0,GEN=0,",),
      coverage=dict(clips=3))

# 3! is no power of two: the float64 division of the integrator term
_case("o3_fact6",
      _base(2, transition_dynamics_order=3, time_unit=0.5, state_space_max=1, action_space_max=1,
            target_point=[0.3, -0.2], target_radius=0.05),
      rollout=("k_continuous_rollout_fast<D=2,ORDER=3,NREL=2,NOISE=0,HELPER=0,GEN=0,",),
      step=("k_continuous_step1<D=2,ORDER=3,NREL=2,NOISE=0,GEN=0,",),
      coverage=dict(clips=3))

# a delay line and an every-n mask: the reward changes between np.float32 and Python-float arithmetic (GEN = 1)
_case("d4_prefix_gen",
      _base(4, relevant_indices=[0, 1], irrelevant_features=True, transition_dynamics_order=2, inertia=2.0, time_unit=0.5,
            state_space_max=1, action_space_max=1, target_point=[0.25, -0.5], target_radius=0.1, delay=2,
            reward_every_n_steps=2, reward_scale=1.5, reward_shift=-0.25, term_state_reward=-1.0),
      rollout=("k_continuous_rollout_fast<D=4,ORDER=2,NREL=2,NOISE=0,HELPER=0,GEN=1,",),
      step=("k_continuous_step1<D=4,ORDER=2,NREL=2,NOISE=0,GEN=1,",),
      coverage=dict(clips=3))

# both noise keys present at 0: the draws advance the stream, the noise term is +0.0.  The generator / walker / consumer
# form (Z0) needs whole 256-env blocks, so this case runs at N = 512 too.
_case("d2_sigma0",
      _base(2, state_space_max=4, action_space_max=1, target_point=[0.5, -1.0], target_radius=0.05, transition_noise=0.0,
            reward_noise=0.0),
      Ns=(300, 512),
      rollout={300: ("k_continuous_rollout_fast<D=2,ORDER=1,NREL=2,NOISE=1,HELPER=0,GEN=0,PHILOX=0,",),
               512: ("k_continuous_rollout_fast<D=2,ORDER=1,NREL=2,NOISE=1,HELPER=1,GEN=0,PHILOX=0,NPROD=2,Z0=1>",)},
      step={300: ("k_continuous_rollout_fast<D=2,ORDER=1,NREL=2,NOISE=1,HELPER=0,",),
            512: ("k_continuous_step1<D=2,ORDER=1,NREL=2,NOISE=1,GEN=0,PHILOX=0,WG=256>",)},
      coverage=dict(clips=3, on_wall_unclipped=0))

# the BASELINE cfg 5 shape in a box small enough for the wall run, on both kinds of streams
_case("d12_noise",
      _base(12, relevant_indices=[0, 1, 2, 3], irrelevant_features=True, transition_dynamics_order=2, time_unit=0.1,
            state_space_max=0.25, action_space_max=1, target_point=[0, 0, 0, 0], target_radius=0.05, transition_noise=0.05,
            reward_noise=0.05),
      rngs=("numpy", "philox"), Ns=(300, 512),
      rollout={("numpy", 300): ("k_continuous_rollout_fast<D=12,ORDER=2,NREL=4,NOISE=1,HELPER=0,GEN=0,PHILOX=0,",),
               ("numpy", 512): ("k_continuous_rollout_fast<D=12,ORDER=2,NREL=4,NOISE=1,HELPER=1,GEN=0,PHILOX=0,NPROD=2>",),
               ("philox", 300): ("k_continuous_rollout_fast<D=12,ORDER=2,NREL=4,NOISE=1,HELPER=0,GEN=0,PHILOX=1,",),
               ("philox", 512): ("k_continuous_rollout_fast<D=12,ORDER=2,NREL=4,NOISE=1,HELPER=1,GEN=0,PHILOX=1,",)},
      step={("numpy", 300): ("k_continuous_rollout_fast<D=12,ORDER=2,NREL=4,NOISE=1,HELPER=0,",),
            ("numpy", 512): ("k_continuous_step1<D=12,ORDER=2,NREL=4,NOISE=1,GEN=0,PHILOX=0,PAR=1>",),
            ("philox", 300): ("k_continuous_step1<D=12,ORDER=2,NREL=4,NOISE=1,GEN=0,PHILOX=1,",),
            ("philox", 512): ("k_continuous_step1<D=12,ORDER=2,NREL=4,NOISE=1,GEN=0,PHILOX=1,",)},
      coverage=dict(clips=3))

# a bounded state box with the default, unbounded action box: +-inf and actions whose square overflows are ADMITTED, and
# action_loss_weight * norm(action) is 0 * inf = NaN there even at weight 0
for _o in (1, 2):
    for _w in (0.0, 0.01):
        _case("amax_inf_o%d_w%s" % (_o, "0" if _w == 0.0 else "01"),
              _base(2, transition_dynamics_order=_o, time_unit=1.0 if _o == 1 else 0.5, state_space_max=4,
                    target_point=[1.0, -2.0], target_radius=0.05, make_denser=_w == 0.0, action_loss_weight=_w,
                    reward_scale=1.5, reward_shift=0.125),
              body="unbounded",
              # (weight 0: the fused kernels would skip the penalty, so the dispatch keeps such a handle on the general kernel)
              rollout=("k_continuous_rollout_fast<D=2,ORDER=%d,NREL=2,NOISE=0,HELPER=0,GEN=0," % _o if _w else "k_continuous_step<DMAX=2,OMAX=2,",),
              step=("k_continuous_step1<D=2,ORDER=%d,NREL=2,NOISE=0,GEN=0," % _o if _w else "k_continuous_step<DMAX=2,OMAX=2,",),
              coverage=dict(clips=3, nan_rewards=3))

# a bounded action box whose corners have squares beyond float32: the same 0 * inf with finite actions
_case("amax_2e19",
      _base(2, state_space_max=4, action_space_max=2e19, target_point=[1.0, -2.0], target_radius=0.05),
      rollout=("k_continuous_step<DMAX=2,OMAX=2,",), step=("k_continuous_step<DMAX=2,OMAX=2,",),
      coverage=dict(clips=3, nan_rewards=3))

# the default, unbounded state box with bounded actions: reset() samples normals, nothing is ever clipped
_case("smax_inf",
      _base(2, transition_dynamics_order=2, time_unit=0.5, action_space_max=1, target_point=[0.5, 0.5], target_radius=0.05),
      rollout=("k_continuous_rollout_fast<D=2,ORDER=2,NREL=2,NOISE=0,HELPER=0,GEN=1,",),
      step=("k_continuous_step1<D=2,ORDER=2,NREL=2,NOISE=0,GEN=1,",))

# both boxes unbounded (the library's defaults): inf followed by -inf makes a NaN coordinate, which np.clip keeps, and the
# reference pays no reward while coordinate 0 of the state it left is NaN (rl_toy_env.py:1858).  The general kernel only.
_case("both_inf",
      _base(2, target_point=[0.5, 0.5], target_radius=0.05, reward_scale=1.5, reward_shift=0.125, delay=1),
      body="unbounded",
      rollout=("k_continuous_step<DMAX=2,OMAX=2,PHILOX=0>",), step=("k_continuous_step<DMAX=2,OMAX=2,PHILOX=0>",),
      coverage=dict(nan_rewards=3, nan_states=3))

_LINE = dict(reward_function="move_along_a_line", state_space_max=4, action_space_max=1, reward_scale=1.5, reward_shift=0.25)
_case("line_d2_l4", _base(2, sequence_length=4, **_LINE), body="line", line=True, max_episode_steps=32,
      rollout=("k_continuous_line_rollout<D=2,ORDER=1,PHILOX=0>",), step=("k_continuous_step<DMAX=2,OMAX=2,PHILOX=0>",),
      coverage=dict(clips=3, on_wall_unclipped=0))
_case("line_d4_o2_l3", _base(4, sequence_length=3, transition_dynamics_order=2, **dict(_LINE, time_unit=0.5)), body="line",
      line=True, max_episode_steps=32,
      rollout=("k_continuous_line_rollout<D=4,ORDER=2,PHILOX=0>",), step=("k_continuous_step<DMAX=4,OMAX=2,PHILOX=0>",),
      coverage=dict(clips=3))

POINT_CASES = [n for n in CASES if not CASES[n]["line"]]
LINE_CASES = [n for n in CASES if CASES[n]["line"]]


def variants(name):
    """(autoreset, rng, N) of every run of a case."""
    c = CASES[name]
    return [(ar, rng, N) for ar in c["autoreset"] for rng in c["rngs"] for N in c["Ns"]]


def expected_names(name, rng, N):
    """(substrings of the rollout kernel's name, of the one-step kernel's name) under the default dispatch."""
    c = CASES[name]

    def pick(v):
        if isinstance(v, dict):
            return v[(rng, N)] if (rng, N) in v else v[N]
        return v
    return pick(c["rollout"]), pick(c["step"])


# ------------------------------------------------------------------------------------------------ scripts
def _amax(cfg):
    return float(cfg.get("action_space_max", INF))


def _smax(cfg):
    return float(cfg.get("state_space_max", INF))


def wall_run_steps(cfg):
    """Steps of +action_space_max in every dimension after which an env that started at rest anywhere in the box has been
    clipped onto +state_space_max: the dynamics integrated from -state_space_max (float64 is enough for a step count), one
    more step for the clip itself.  An unbounded action box reaches the wall in one step (+inf); without a wall: 0."""
    smax, amax = _smax(cfg), _amax(cfg)
    if not np.isfinite(smax):
        return 0
    if not np.isfinite(amax):
        return 1
    n, t = int(cfg.get("transition_dynamics_order", 1)), float(cfg.get("time_unit", 1.0))
    sd = [0.0] * (n + 1)
    sd[0] = -smax - 4 * float(cfg.get("transition_noise") or 0.0)       # (noise may push the start back a little)
    fact = [1.0, 1.0, 2.0, 6.0, 24.0]
    steps = 0
    while sd[0] <= smax and steps < T:
        sd[n] = amax / float(cfg.get("inertia", 1.0))
        for i in range(n):
            for j in range(n - i):
                sd[i] += sd[i + j + 1] * t ** (j + 1) / fact[j + 1]
        steps += 1
    return steps + 1


def palette(cfg):
    """(admitted values, rejected values) for one coordinate of an action."""
    amax = _amax(cfg)
    adm = [0.0, -0.0, DENORM_MIN, -DENORM_MIN, DENORM_MAX, -DENORM_MAX, FLT_MIN, -FLT_MIN, 1e-20, -1e-20]   # (1e-20: its square is subnormal)
    rej = [NAN]
    if np.isfinite(amax):
        adm += [amax, -amax]
        out = float(np.nextafter(F32(amax), F32(INF)))
        rej += [out, -out, INF, -INF]
    else:
        adm += [INF, -INF, 3e19, -3e19, FLT_MAX, -FLT_MAX]             # (3e19 ** 2 overflows float32)
    return adm, rej


def _row(D, fill, **at):
    r = [fill] * D
    for d, v in at.items():
        r[int(d[1:])] = v
    return r


def _body_point(cfg, length):
    """Palette values one coordinate at a time among uniform ones, whole rows of +-amax (pushes into the wall and away from
    it), rows with a rejected coordinate, uniform rows."""
    D, amax = int(cfg["state_space_dim"]), _amax(cfg)
    a1 = amax if np.isfinite(amax) else 1.0
    adm, rej = palette(cfg)
    rows, k = [], 0
    while len(rows) < length:
        ph = k % 8
        d = k % D
        if ph == 0:
            rows.append(_row(D, U, **{"d%d" % d: adm[(k // 8) % len(adm)]}))
        elif ph == 1:
            rows.append(_row(D, U, **{"d%d" % d: rej[(k // 8) % len(rej)]}))
        elif ph == 2:
            rows += [_row(D, -a1)] * 2                       # off the wall ...
        elif ph == 3:
            rows += [_row(D, a1)] * 3                        # ... and into it again
        elif ph == 4:
            rows.append(_row(D, adm[(k // 8 + 5) % len(adm)]))     # the same palette value in every coordinate
        elif ph == 5:
            rows.append(_row(D, 0.0, **{"d%d" % d: -a1}))    # one coordinate leaves the wall, the others stay on it
        elif ph == 6:
            rows.append(_row(D, 0.0, **{"d%d" % d: a1}))
        else:
            rows += [_row(D, U)] * 2
        k += 1
    return rows[:length]


def _body_unbounded(cfg, length):
    """The default action box: +-inf, +-FLT_MAX and +-3e19 are admitted.  inf then -inf in one coordinate (a NaN coordinate
    where the state box is unbounded too), the palette, uniform rows."""
    D = int(cfg["state_space_dim"])
    adm, rej = palette(cfg)
    big = [INF, -INF, 3e19, -3e19, FLT_MAX, -FLT_MAX]
    rows, k = [], 0
    while len(rows) < length:
        ph = k % 8
        d = k % D
        if ph == 0:
            rows.append(_row(D, U, **{"d%d" % d: big[(k // 8) % len(big)]}))
        elif ph == 1:
            rows.append(_row(D, U, **{"d%d" % d: -big[(k // 8) % len(big)]}))      # inf, then -inf: NaN without a wall
        elif ph == 2:
            rows.append(_row(D, U, **{"d%d" % d: rej[0]}))
        elif ph == 3:
            rows.append(_row(D, U, **{"d%d" % d: adm[(k // 8) % len(adm)]}))
        elif ph == 4:
            rows.append(_row(D, big[(k // 8 + 1) % len(big)]))
        elif ph == 5:
            rows.append(_row(D, 0.0, **{"d%d" % d: -1.0}))
        else:
            rows += [_row(D, U)] * 2
        k += 1
    return rows[:length]


def _body_lattice(cfg, length):
    """Moves of the integer lattice.  Every cycle starts with (+1, +1) three times: the first (after a next-step reset call:
    the second) takes a fresh state onto the wall next to the corner, the next one onto (4, 4); there they are clips.
    At first cycles that keep an env on (4, 4) and (3, 4) -- off the wall to the radius, back onto the wall without a
    clip, palette values that leave the state where it is -- so that envs reach max_episode_steps; afterwards cycles that
    end on the cube's corner."""
    adm, rej = palette(cfg)
    rows, k = [], 0
    while len(rows) < length:
        keep = [[1.0, 1.0]] * 3 + [[-1.0, 0.0], [1.0, 0.0], [rej[k % len(rej)], 0.0], [adm[k % 10], adm[(k + 3) % 10]],
                                   [-1.0, 0.0], [0.0, rej[(k + 1) % len(rej)]], [1.0, 0.0]]
        rows += keep if len(rows) < 44 else [[1.0, 1.0]] * 3 + [[-1.0, 0.0], [1.0, 0.0], [0.0, -1.0]]
        k += 1
    return rows[:length]


def _body_line(cfg, length):
    """In this order: sequence_length + 2 rejected actions (a stationary window), a slide along the wall, and for the
    rest a zig-zag among uniform rows, with a rejected action and a palette value now and then."""
    D, L = int(cfg["state_space_dim"]), int(cfg["sequence_length"])
    adm, rej = palette(cfg)
    rows = [_row(D, 0.5, d0=rej[k % len(rej)]) for k in range(L + 2)]
    rows += [_row(D, 1.0, d0=-0.75, d1=0.25) for _ in range(L + 3)]       # pressed onto the wall in d >= 2 (d1: drifting into it), sliding back in d0
    k = 0
    while len(rows) < length:
        s = 1.0 if k % 2 == 0 else -1.0
        ph = k % 12
        if ph < 7:                        # d0 turns every third step, the others every step: the window is never collinear
            rows.append([0.7 * (1.0 if k % 6 < 3 else -1.0) if d == 0 else s * (0.9 if d % 2 == 0 else -0.6) for d in range(D)])
        elif ph == 7:
            rows.append(_row(D, U, d0=rej[(k // 12) % len(rej)]))
        elif ph == 8:
            rows.append(_row(D, U, d1=adm[(k // 12) % len(adm)]))
        else:
            rows.append(_row(D, U))
        k += 1
    return rows[:length]


_BODIES = dict(point=_body_point, unbounded=_body_unbounded, lattice=_body_lattice, line=_body_line)


def scripts(name, N, seed=7):
    """float32 [T, N, D]: the case's action script of every env."""
    c = CASES[name]
    cfg = c["config"]
    D, amax = int(cfg["state_space_dim"]), _amax(cfg)
    W = max(wall_run_steps(cfg), c["wall"])
    wall = [[amax] * D] * W
    body = _BODIES[c["body"]](cfg, T - W)
    rng = np.random.default_rng(seed)
    ubound = amax if np.isfinite(amax) else 1.0
    lattice = c["body"] == "lattice"

    def fill(rows, g):
        out = np.empty((len(rows), D), F32)
        for t, r in enumerate(rows):
            for d, v in enumerate(r):
                if v is U:
                    v = float(g.integers(-1, 2)) if lattice else g.uniform(-ubound, ubound)
                out[t, d] = v
        return out
    acts = np.empty((T, N, D), F32)
    shared = fill(wall + body, rng)
    for i in range(N):
        if i < 64:
            acts[:, i] = shared
        else:
            sh = 1 + (5 * i) % (len(body) - 1)
            acts[:, i] = fill(wall + body[sh:] + body[:sh], np.random.default_rng([seed, i]))
    return acts


# ------------------------------------------------------------------------------------------------ trajectories
def admitted(cfg, a):
    """Box.contains(action) for a float32 vector: inclusive bounds, NaN outside."""
    amax = F32(_amax(cfg))
    return bool(np.all(a >= -amax) and np.all(a <= amax))


def drive(env, script, cfg, max_episode_steps, autoreset, launches=LAUNCHES):
    """One env through its script the way RLToyVectorEnv runs it.  `env`: reset() -> obs (the explicit reset),
    auto_reset() -> obs, step(a) -> (obs, reward, done), derivs() -> [order + 1, D], streams() -> (env words, space words).
    Returns per-step arrays -- "obs" (after a same-step autoreset: the new episode's first observation), "final" (the
    observation before that reset), "reward" (float32), "term", "trunc", "reset_call" (next-step autoreset: this call was
    the reset), "bad" (a rejected action; not on a reset call), "derivs_pre" (before any autoreset) -- and per launch
    "derivs" and "streams" as they stand after it."""
    n_steps, D = script.shape
    assert sum(launches) == n_steps
    order = int(cfg.get("transition_dynamics_order", 1))
    out = dict(init=np.array(env.reset(), F32), obs=np.zeros((n_steps, D), F32), final=np.zeros((n_steps, D), F32),
               reward=np.zeros(n_steps, F32), term=np.zeros(n_steps, bool), trunc=np.zeros(n_steps, bool),
               reset_call=np.zeros(n_steps, bool), bad=np.zeros(n_steps, bool),
               derivs_pre=np.zeros((n_steps, order + 1, D), F32), derivs=[], streams=[])
    n, pending, t = 0, False, 0
    for K in launches:
        for _ in range(K):
            if pending:                       # gymnasium's next-step autoreset: the action is ignored, reward 0, no flags
                out["obs"][t] = env.auto_reset()
                out["final"][t] = out["obs"][t]
                out["reset_call"][t] = True
                out["derivs_pre"][t] = env.derivs()
                n, pending = 0, False
                t += 1
                continue
            a = script[t]
            o, r, d = env.step(a)
            n += 1
            tr = max_episode_steps > 0 and n >= max_episode_steps
            out["final"][t] = o
            out["derivs_pre"][t] = env.derivs()
            out["reward"][t] = F32(r)
            out["term"][t], out["trunc"][t] = d, tr
            out["bad"][t] = not admitted(cfg, a)
            if d or tr:
                if autoreset == "same_step":
                    o = env.auto_reset()
                    n = 0
                elif autoreset == "next_step":
                    pending = True
            out["obs"][t] = o
            t += 1
        out["derivs"].append(np.array(env.derivs(), F32))
        out["streams"].append(env.streams())
    return out


def coverage(name, traj, script):
    """Event counts of one env's trajectory (see the module docstring), from the oracle's outputs alone."""
    cfg = CASES[name]["config"]
    smax, order = F32(_smax(cfg)), int(cfg.get("transition_dynamics_order", 1))
    inertia = F32(cfg.get("inertia", 1.0))
    rel = list(cfg.get("relevant_indices", range(int(cfg["state_space_dim"]))))
    live = ~traj["reset_call"]
    adm = live & ~traj["bad"]
    # a clip zeroes EVERY derivative, the highest (action / inertia) included; without one that row is the action's
    moved = np.array([np.any(F32(a) / inertia != 0) for a in script])
    clip = adm & moved & np.all(traj["derivs_pre"][:, 1:] == 0, axis=(1, 2))
    prev = np.concatenate([traj["init"][None], traj["obs"][:-1]])
    arrive = np.any((np.abs(traj["final"]) == smax) & (np.abs(prev) != smax), axis=1) if np.isfinite(smax) else np.zeros(len(clip), bool)
    c = dict(clips=int(clip.sum()), on_wall_unclipped=int((adm & ~clip & arrive).sum()), rejected=int((live & traj["bad"]).sum()),
             truncations=int(traj["trunc"].sum()), nan_rewards=int(np.isnan(traj["reward"]).sum()),
             nan_states=int((live & np.isnan(traj["final"]).any(axis=1)).sum()), at_radius=0, cube_face=0)
    if not CASES[name]["line"]:
        tgt = np.asarray(cfg["target_point"], F32)
        diff = traj["final"][:, rel] - tgt
        with np.errstate(over="ignore", invalid="ignore"):
            dist = np.sqrt((diff * diff).astype(np.float64).sum(axis=1).astype(F32))      # float32 products, a float64 sum, a float32 root
        c["at_radius"] = int((live & (dist == F32(cfg["target_radius"]))).sum())
        if "terminal_states" in cfg:
            e = cfg["term_state_edge"]
            for centre in cfg["terminal_states"]:
                lo, hi = np.asarray(centre, F32) - F32(e / 2), np.asarray(centre, F32) + F32(e / 2)
                x = traj["final"][:, rel]
                inside = np.all((x >= lo) & (x <= hi), axis=1)
                on_face = np.any((x == lo) | (x == hi), axis=1)
                c["cube_face"] += int((live & traj["term"] & inside & on_face & (dist >= F32(cfg["target_radius"]))).sum())
    return c
