"""Construction time of RLToyVectorEnv(seeds=[...]) -- one MDP per env -- on the host path against the device generator
(mdpp_generate.hip), at 8 192 and 65 536 envs, for cfg2, an S = 50 sequence_length 1 shape and diameter 2.

    python tools/time_mdp_build.py [--sizes 8192,65536] [--host-sample 2048] [--out profiles/device_mdp_build.json]

host:   mdp.build_mdp({**config, "seed": s}) in one process, timed on the first --host-sample seeds and scaled to N (the
        builds are independent and equally expensive), plus the per-env stream seeding the host path adds
        (one new_generator per env and stream).  0 = time all N.
device: the whole constructor (env 0 built on the host, handle, one generator launch, stream read-back, first reset),
        ended by torch.cuda.synchronize(); and within it mdpp_generate_discrete alone.  The best of --repeats runs,
        after a small warm-up construction that loads the code objects.
"""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mdp_playground_amd import RLToyVectorEnv, mdp  # noqa: E402
from mdp_playground_amd import vector_env  # noqa: E402

BASE = dict(state_space_type="discrete", action_space_type="discrete")
CONFIGS = {
    "cfg2": dict(BASE, state_space_size=8, action_space_size=8, delay=4, sequence_length=3),
    "s50_l1": dict(BASE, state_space_size=50, action_space_size=50, sequence_length=1),
    "diameter2": dict(BASE, action_space_size=8, diameter=2, sequence_length=2),
}


def host_seconds(cfg, N, sample):
    n = N if sample <= 0 else min(N, sample)
    t0 = time.perf_counter()
    for s in range(n):
        m = mdp.build_mdp({**cfg, "seed": s})
        mdp.pcg64_words(mdp.new_generator(m.seed_dict["env"]))       # the env stream _seed_streams seeds per env
    return (time.perf_counter() - t0) * N / n


def device_seconds(cfg, N, dev, repeats):
    gen_s = []
    orig = vector_env.RLToyVectorEnv._generate_discrete

    def timed(self):
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        orig(self)
        torch.cuda.synchronize(dev)
        gen_s.append(time.perf_counter() - t)

    vector_env.RLToyVectorEnv._generate_discrete = timed
    best = None
    try:
        for _ in range(repeats):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            env = RLToyVectorEnv(seeds=list(range(N)), device=dev, **cfg)
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t0
            assert env.tables_built_on == "device"
            env.close()
            best = dt if best is None else min(best, dt)
    finally:
        vector_env.RLToyVectorEnv._generate_discrete = orig
    return best, min(gen_s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8192,65536")
    ap.add_argument("--host-sample", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    warnings.simplefilter("ignore")
    dev = torch.device("cuda", 0)
    RLToyVectorEnv(seeds=[0, 1], device=dev, **CONFIGS["cfg2"]).close()      # warm-up: code objects, allocator
    rows = []
    for name, cfg in CONFIGS.items():
        for N in (int(x) for x in args.sizes.split(",")):
            h = host_seconds(cfg, N, args.host_sample)
            d, g = device_seconds(cfg, N, dev, args.repeats)
            row = dict(config=name, num_envs=N, host_s=round(h, 3), host_sampled=min(N, args.host_sample) if args.host_sample > 0 else N,
                       device_ctor_s=round(d, 4), device_generate_s=round(g, 4), speedup=round(h / d, 1))
            print(json.dumps(row), flush=True)
            rows.append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(dev), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
