"""The cases of the grid learners' tests (tests/test_grid_learner_host.py runs each on the CPU and asserts the conditions that
keep a GPU pass honest; tests/test_gpu_grid_learn.py runs each on the GPU against tests/grid_learner_ref.py).

The smallest shapes that can still go wrong: (3, 4) non-square, so a transposed index shows (QLDS=1); (5, 5) with four
actions, the largest square grid whose 256 tables fit in LDS (36 x 4 x 1 KiB = 144 KiB), and with the noop the same grid
in global memory (180 KiB does not fit); (1, 7), a dimension whose only in-grid cell is 0; (8, 8), QLDS=0.  Between them:
dense and sparse rewards, with and without max_episode_steps, the three autoreset modes, every-n = 3 with scale, shift and
terminal reward, both noise keys, int32 observations.

N = 320 is one full workgroup plus one wave: lanes past N exist.  K = 37 is no multiple of 4 (the learner's words come in
blocks of four ticks), two launches cross a launch boundary with a SARSA carry pending."""
import numpy as np

N, K, LAUNCHES = 320, 37, 2
PHILOX_SEED, ENV_ID_OFFSET, LEARNER_SEED = 41, 1000, 0xFEEDFACE12345

_BASE = dict(state_space_type="grid", reward_function="move_to_a_point", seed=5)

CASES = {
    # name: config, handle kwargs, noop, the table placement the launch must report, (alpha, gamma, epsilon), random initial tables
    "g34_dense": dict(cfg=dict(_BASE, grid_shape=(3, 4), make_denser=True, target_point=[1, 2]),
                      kw=dict(autoreset="same_step"), noop=False, qlds=1, rates=(0.5, 0.9, 0.3), q0=False),
    "g55_sparse_limit_i32": dict(cfg=dict(_BASE, grid_shape=(5, 5), make_denser=False, target_point=[3, 1], dtype_s=np.int32),
                                 kw=dict(autoreset="same_step", max_episode_steps=9), noop=False, qlds=1, rates=(0.25, 0.95, 0.4), q0=True),
    "g55_noop_next_every3": dict(cfg=dict(_BASE, grid_shape=(5, 5), make_denser=True, target_point=[2, 2], reward_every_n_steps=3,
                                          reward_scale=1.5, reward_shift=-0.125, term_state_reward=2.0),
                                 kw=dict(autoreset="next_step", max_episode_steps=7), noop=True, qlds=0, rates=(0.5, 0.75, 0.35), q0=True),
    "g17_noise": dict(cfg=dict(_BASE, grid_shape=(1, 7), make_denser=True, target_point=[0, 4], transition_noise=0.3, reward_noise=0.5),
                      kw=dict(autoreset="same_step", max_episode_steps=11), noop=False, qlds=1, rates=(0.5, 0.9, 0.3), q0=False),
    "g88_disabled_pnoise": dict(cfg=dict(_BASE, grid_shape=(8, 8), make_denser=False, target_point=[1, 1], transition_noise=0.25,
                                         term_state_reward=-0.5),
                                kw=dict(autoreset="disabled", max_episode_steps=29), noop=False, qlds=0, rates=(0.75, 0.5, 0.5), q0=True),
    "g34_noise_next_i32": dict(cfg=dict(_BASE, grid_shape=(3, 4), make_denser=False, target_point=[2, 0], transition_noise=0.2,
                                        reward_noise=0.25, reward_scale=2.0, dtype_s=np.int32),
                               kw=dict(autoreset="next_step", max_episode_steps=6), noop=True, qlds=1, rates=(0.5, 0.9, 0.3), q0=False),
}


def n_actions(case):
    return 5 if CASES[case]["noop"] else 4


def initial_tables(case, n=N):
    """float32 [n, S, A]: the case's initial tables (None: zeros) -- small values of both signs, ties included"""
    c = CASES[case]
    if not c["q0"]:
        return None
    g = c["cfg"]["grid_shape"]
    r = np.random.default_rng(sorted(CASES).index(case) + 100)
    return (r.integers(-3, 4, size=(n, (g[0] + 1) * (g[1] + 1), n_actions(case))) * 0.125).astype(np.float32)


_cpu_runs = {}


def cpu_run(case, algo, streams=None):
    """(info, Q, traj) of the case's two learning launches on the CPU (tests/grid_learner_ref.closed_loop), computed once per
    (case, algo) on the Philox streams of the cases' key; with ``streams`` (a handle's seeded numpy words) computed afresh"""
    import grid_learner_ref as gref
    c = CASES[case]
    al, ga, ep = c["rates"]

    def run():
        return gref.closed_loop(c["cfg"], c["kw"], algo, al, ga, ep, N, initial_tables(case), seed=LEARNER_SEED, K=K, launches=LAUNCHES,
                                noop=c["noop"], philox_seed=PHILOX_SEED, off=ENV_ID_OFFSET, streams=streams)
    if streams is not None:
        return run()
    if (case, algo) not in _cpu_runs:
        _cpu_runs[case, algo] = run()
    return _cpu_runs[case, algo]


def expected_name(case, rng, eval=False, summary=False, qlds=None):
    c = CASES[case]
    noise = int("transition_noise" in c["cfg"] or "reward_noise" in c["cfg"])
    return "k_grid_learn_rollout<PHILOX=%d,NOISE=%d,QLDS=%d,EVAL=%d,SUMMARY=%d>" % (
        int(rng == "philox"), noise, c["qlds"] if qlds is None else qlds, int(eval), int(summary))
