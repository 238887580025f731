"""A seeded random family of discrete configs that mdp.device_coverage accepts: what the device MDP generator
(mdpp_generate.hip) is tested on, through its host build (test_mdp_generate_host.py) and on the device
(test_gpu_device_mdp.py).  Draws are made by rejection until the coverage rule accepts them; a second rejection keeps
each config cheap enough to check against mdp.build_mdp in a test.  classes() names the corners of the rule each config
reaches, and MIN_CLASS_COUNTS is how often every one must appear in family(FAMILY_SIZE)."""
import numpy as np

from mdp_playground_amd import mdp

BASE = dict(state_space_type="discrete", action_space_type="discrete")

TERM_DENSITIES = (0.0, 0.1, 0.25, 0.5, 0.9)
# (0.02 as well: with a sequence-number population above 10 000, n_sel == total // 50 is the last Floyd pick count)
REWARD_DENSITIES = (0.0, 1e-6, 0.01, 0.02, 0.25, 1.0)

# what a config may cost a test: the dense reward table of one env (bits with unit rewards, float64 values otherwise),
# the bitset of `total` bits the generator clears per env, and the sequences build_mdp decodes in Python
MAX_KEYS_UNIT = 1 << 28
MAX_KEYS_VALUES = 1 << 22
MAX_TOTAL = 1 << 30
MAX_SEQS = 4000

# the exact Floyd-branch edges of Generator.choice(total, n_sel, replace=False)
FLOYD_EDGES = {
    "floyd_total_10000": dict(BASE, action_space_size=13, sequence_length=4, repeats_in_sequences=True),
    "floyd_nsel_total_div_50": dict(BASE, action_space_size=14, sequence_length=4, repeats_in_sequences=True,
                                    reward_density=0.02),
}

FAMILY_SIZE = 320
FAMILY_SEED = 20261016

MIN_CLASS_COUNTS = {
    "total>10000": 40,
    "n_sel==total//50": 8,
    "L>=8": 40,
    "repeats,L>=5": 30,
    "diameter>=3": 40,
    "diameter>=8": 1,
    "A==1": 4,
    "n_term==0": 40,
    "n_sel==1": 30,
    "values,diameter>1": 20,
    # what only the order of the picks decides: the values they get, or a later draw from the same generator
    "total>10000,order-sensitive": 15,
    "S==255": 2,
    "keys>2^24": 10,
    "not maximally_connected": 30,
    "make_denser": 30,
    "image": 8,
    "transition_noise": 15,
    "reward_dist=[1,1]": 15,
}


def classes(cfg):
    p = mdp.device_gen_params(cfg)
    S, L, d, total, n_sel = p["S"], p["L"], p["diameter"], p["total"], p["n_sel"]
    out = set()
    if total > 10000:
        out.add("total>10000")
        if p["rews"] is not None or (d > 1 and not p["repeats"]):
            out.add("total>10000,order-sensitive")
    if total > 10000 and n_sel == total // 50:
        out.add("n_sel==total//50")
    if L >= 8:
        out.add("L>=8")
    if p["repeats"] and L >= 5:
        out.add("repeats,L>=5")
    if d >= 3:
        out.add("diameter>=3")
    if d >= 8:
        out.add("diameter>=8")
    if p["A"] == 1:
        out.add("A==1")
    if p["n_term"] == 0:
        out.add("n_term==0")
    if n_sel == 1:
        out.add("n_sel==1")
    if not p["unit_rewards"] and d > 1:
        out.add("values,diameter>1")
    if S == 255:
        out.add("S==255")
    if S ** L > 1 << 24:
        out.add("keys>2^24")
    if not p["maximally_connected"]:
        out.add("not maximally_connected")
    if cfg.get("make_denser"):
        out.add("make_denser")
    if p["image"]:
        out.add("image")
    if cfg.get("transition_noise"):
        out.add("transition_noise")
    if cfg.get("reward_dist") == [1.0, 1.0]:
        out.add("reward_dist=[1,1]")
    return out


def affordable(cfg):
    """An env of the config can be made (mdpp_create: at least 2 states, L <= 7 with image observations), and its
    tables and host build stay small enough for a test (the MAX_* limits above)."""
    p = mdp.device_gen_params(cfg)
    if p["S"] < 2 or (p["image"] and p["L"] > 7):
        return False
    keys = p["S"] ** p["L"]
    if keys > (MAX_KEYS_UNIT if p["unit_rewards"] else MAX_KEYS_VALUES):
        return False
    return p["total"] <= MAX_TOTAL and p["diameter"] * p["n_sel"] <= MAX_SEQS


def _draw(r):
    u = r.random()
    d = int(r.integers(5, 17)) if u < 0.03 else int(r.choice([1, 1, 1, 2, 2, 3, 4]))
    L = int(r.integers(1, 16))
    # A: log-uniform over 2 .. the largest A whose S^L keys stay affordable (all of 1 .. 255 // d one time in ten), with
    # 1 and the top drawn now and then
    top = 255 // d if r.random() < 0.1 else max(1, min(255 // d, int(MAX_KEYS_UNIT ** (1.0 / L)) // d))
    v = r.random()
    A = 1 if v < 0.02 else top if v < 0.1 else int(np.exp(r.uniform(np.log(2), np.log(top + 1))))
    A = min(max(A, 1), top)
    cfg = dict(BASE, action_space_size=A, diameter=d, sequence_length=L,
               terminal_state_density=float(r.choice(TERM_DENSITIES)),
               reward_density=float(r.choice(REWARD_DENSITIES)))
    if r.random() < 0.5:
        cfg["repeats_in_sequences"] = True
    if r.random() < 0.2:
        cfg["maximally_connected"] = False
    if r.random() < 0.2:
        cfg["make_denser"] = True
    w = r.random()
    if w < 0.3:
        cfg["reward_dist"] = [float(np.round(r.uniform(-1.0, 0.9), 3)), 1.0]
    elif w < 0.45:
        cfg["reward_dist"] = [1.0, 1.0]
    if A * d <= 32 and r.random() < 0.1:
        cfg.update(image_representations=True, image_width=32, image_height=32)
    if r.random() < 0.12:
        cfg["transition_noise"] = 0.1
    if r.random() < 0.12:
        cfg["reward_noise"] = 0.5
    return cfg


def family(n=FAMILY_SIZE, seed=FAMILY_SEED):
    """[(name, config)]: the FLOYD_EDGES configs, then n - len(FLOYD_EDGES) random covered, affordable configs."""
    out = list(FLOYD_EDGES.items())
    r = np.random.default_rng(seed)
    while len(out) < n:
        cfg = _draw(r)
        if mdp.device_coverage(cfg, [0])[0] and affordable(cfg):
            out.append((f"f{len(out):03d}", cfg))
    return out


def class_counts(configs):
    counts = dict.fromkeys(MIN_CLASS_COUNTS, 0)
    for _, cfg in configs:
        for c in classes(cfg):
            counts[c] += 1
    return counts


# reward tables above this many keys are compared key by key: a dense float64 table of every env would not fit
DENSE_KEYS = 1 << 16


def expected_rewards(m):
    """(keys, values) of m's full-length rewardable sequences, key = sum seq[i] S^(L-1-i) as in reward_table()."""
    L, S = m.sequence_length, m.S
    keys, vals = [], []
    for seq, v in m.rewardable_sequences.items():
        if len(seq) == L:
            k = 0
            for s in seq:
                k = k * S + int(s)
            keys.append(k)
            vals.append(v)
    return np.array(keys, dtype=np.int64), np.array(vals, dtype=np.float64)


def assert_reward_row(m, rbits=None, rtable=None, tag=None):
    """One env's reward table as the kernels read it -- rbits (unit rewards) or rtable -- equals m's: whole up to
    DENSE_KEYS keys, else as the set of keys holding a bit / a non-zero value plus the value at every rewardable key."""
    if m.S ** m.sequence_length <= DENSE_KEYS:
        t = m.reward_table()
        if rbits is not None:
            assert np.array_equal(rbits, np.packbits((t != 0).astype(np.uint8), bitorder="little")), tag
        else:
            assert np.array_equal(rtable, t), tag
        return
    keys, vals = expected_rewards(m)
    if rbits is not None:
        nz = np.flatnonzero(rbits)
        bits = np.unpackbits(rbits[nz], bitorder="little").reshape(-1, 8).astype(bool)
        got = (nz[:, None] * 8 + np.arange(8))[bits]
        assert np.all(vals == 1.0), tag
        assert np.array_equal(np.sort(got), np.sort(keys)), tag
    else:
        got = np.flatnonzero(rtable)
        assert np.array_equal(got, np.sort(keys[vals != 0.0])), tag
        assert np.array_equal(rtable[keys], vals), tag
