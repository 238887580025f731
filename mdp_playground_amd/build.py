"""Build libmdpp_hip.so (the HIP kernels + C ABI) in-tree for gfx950.

    python -m mdp_playground_amd.build [--force]

hipcc cross-compiles without a GPU.  -ffp-contract=off is REQUIRED: the float32/float64
arithmetic of the continuous kernel must not be fused into FMAs (parity with numpy).
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(CSRC, "libmdpp_hip.so")
SOURCES = ["mdpp_capi.hip", "mdpp_discrete.hip", "mdpp_discrete_wide.hip", "mdpp_discrete_long.hip", "mdpp_discrete_fast.hip", "mdpp_discrete_step1.hip", "mdpp_discrete_pipe.hip", "mdpp_discrete_lean.hip", "mdpp_discrete_lean_next.hip", "mdpp_discrete_lean_noise.hip", "mdpp_discrete_lean_npnoise.hip",
           "mdpp_discrete_quiet.hip", "mdpp_discrete_quiet_nu.hip", "mdpp_discrete_policy.hip", "mdpp_discrete_learn.hip",
           "mdpp_discrete_learn_pe.hip", "mdpp_discrete_learn_double.hip", "mdpp_discrete_learn_double_pe.hip",
           "mdpp_discrete_learn_summary.hip", "mdpp_discrete_learn_pe_summary.hip", "mdpp_discrete_learn_double_summary.hip",
           "mdpp_discrete_learn_double_pe_summary.hip", "mdpp_discrete_eval.hip", "mdpp_discrete_eval_summary.hip",
           "mdpp_discrete_learn_pe_nlev.hip", "mdpp_discrete_learn_double_pe_nlev.hip", "mdpp_discrete_learn_pe_nlev_summary.hip",
           "mdpp_discrete_learn_double_pe_nlev_summary.hip", "mdpp_discrete_eval_nlev.hip", "mdpp_discrete_eval_nlev_summary.hip",
           "mdpp_discrete_learn_pe_pm.hip", "mdpp_discrete_learn_double_pe_pm.hip", "mdpp_discrete_learn_pe_pm_summary.hip",
           "mdpp_discrete_learn_double_pe_pm_summary.hip", "mdpp_discrete_eval_pm.hip", "mdpp_discrete_eval_pm_summary.hip",
           "mdpp_discrete_learn_pe_pm_nlev.hip", "mdpp_discrete_learn_double_pe_pm_nlev.hip", "mdpp_discrete_learn_pe_pm_nlev_summary.hip",
           "mdpp_discrete_learn_double_pe_pm_nlev_summary.hip", "mdpp_discrete_eval_pm_nlev.hip", "mdpp_discrete_eval_pm_nlev_summary.hip",
           "mdpp_discrete_learn_pe_sched.hip", "mdpp_discrete_learn_pe_sched_summary.hip", "mdpp_discrete_learn_double_pe_sched.hip",
           "mdpp_discrete_learn_double_pe_sched_summary.hip",
           "mdpp_discrete_learn_pe_nlev_sched.hip", "mdpp_discrete_learn_pe_nlev_sched_summary.hip", "mdpp_discrete_learn_double_pe_nlev_sched.hip",
           "mdpp_discrete_learn_double_pe_nlev_sched_summary.hip", "mdpp_discrete_learn_pe_pm_sched.hip", "mdpp_discrete_learn_pe_pm_sched_summary.hip",
           "mdpp_discrete_learn_double_pe_pm_sched.hip", "mdpp_discrete_learn_double_pe_pm_sched_summary.hip",
           "mdpp_discrete_learn_pe_pm_nlev_sched.hip", "mdpp_discrete_learn_pe_pm_nlev_sched_summary.hip",
           "mdpp_discrete_learn_double_pe_pm_nlev_sched.hip", "mdpp_discrete_learn_double_pe_pm_nlev_sched_summary.hip",
           "mdpp_discrete_trace.hip", "mdpp_discrete_trace_pe.hip", "mdpp_discrete_summary_trace.hip", "mdpp_discrete_summary_trace_pe.hip",
           "mdpp_discrete_trace_pe_sched.hip", "mdpp_discrete_summary_trace_pe_sched.hip",
           "mdpp_discrete_lambda_pe_pm.hip", "mdpp_discrete_summary_lambda_pe_pm.hip",
           "mdpp_discrete_lambda_pe_pm_sched.hip", "mdpp_discrete_summary_lambda_pe_pm_sched.hip",
           "mdpp_continuous.hip", "mdpp_continuous_line8.hip", "mdpp_continuous_linear.hip", "mdpp_continuous_summary_linear.hip",
           "mdpp_continuous_search.hip", "mdpp_continuous_summary_search.hip",
           "mdpp_continuous_es.hip", "mdpp_continuous_summary_es.hip",
           "mdpp_continuous_linear_h2.hip", "mdpp_continuous_summary_linear_h2.hip", "mdpp_continuous_search_h2.hip",
           "mdpp_continuous_summary_search_h2.hip", "mdpp_continuous_es_h2.hip", "mdpp_continuous_summary_es_h2.hip",
           "mdpp_continuous_fast.hip", "mdpp_continuous_step1.hip", "mdpp_continuous_line.hip", "mdpp_image.hip", "mdpp_grid.hip", "mdpp_grid_learn.hip", "mdpp_grid_summary_learn.hip",
           "mdpp_grid_sched_learn.hip", "mdpp_grid_summary_sched_learn.hip", "mdpp_grid_episodes_learn.hip", "mdpp_grid_episodes_sched_learn.hip",
           "mdpp_grid_levels_learn.hip", "mdpp_grid_summary_levels_learn.hip", "mdpp_grid_levels_sched_learn.hip", "mdpp_grid_summary_levels_sched_learn.hip",
           "mdpp_grid_episodes_levels_learn.hip", "mdpp_grid_episodes_levels_sched_learn.hip", "mdpp_imagec.hip", "mdpp_post.hip", "mdpp_peer.hip",
           "mdpp_generate.hip"]
HEADERS = ["mdpp_internal.hpp", "mdpp_rng.hpp", "mdpp_discrete_closed.hpp", "mdpp_pcg64_limbs.inc", "np_ziggurat_tables.inc", "mdpp_grid_learn_body.inc",
           os.path.join("..", "..", "include", "mdpp.h")]
_CLOSED_DEPS = ["mdpp_continuous_closed.hpp", "mdpp_linear_history.hpp"]
_LEAN_DEPS = ["mdpp_discrete_lean.hip", "mdpp_discrete_lean_e.inc"]      # (the kernel and its E role, included into its body)
INCLUDED_SOURCES = {"mdpp_discrete_lean.hip": ["mdpp_discrete_lean_e.inc"], "mdpp_discrete_wide.hip": ["mdpp_discrete.hip"], "mdpp_discrete_long.hip": ["mdpp_discrete.hip"], "mdpp_discrete_lean_next.hip": _LEAN_DEPS, "mdpp_discrete_lean_noise.hip": _LEAN_DEPS, "mdpp_discrete_lean_npnoise.hip": _LEAN_DEPS,
                    "mdpp_continuous_line8.hip": ["mdpp_continuous.hip"], "mdpp_continuous_step1.hip": ["mdpp_continuous_fast.hip"], "mdpp_discrete_quiet_nu.hip": ["mdpp_discrete_quiet.hip"],   # a .hip that #includes another one
                    # ... or a header of its own
                    **{u: ["mdpp_discrete_learn.hpp"] for u in SOURCES if u.startswith("mdpp_discrete_learn")},
                    **{u: ["mdpp_discrete_eval.hpp"] for u in SOURCES if u.startswith("mdpp_discrete_eval")},
                    **{u: ["mdpp_discrete_trace.hpp", "mdpp_discrete_learn.hpp"] for u in SOURCES if u.startswith(("mdpp_discrete_trace", "mdpp_discrete_summary_trace"))},
                    # (... on one MDP per env: the same header's PM forms)
                    **{u: ["mdpp_discrete_trace.hpp", "mdpp_discrete_learn.hpp"] for u in SOURCES if u.startswith(("mdpp_discrete_lambda", "mdpp_discrete_summary_lambda"))},
                    # the grid learners' two output forms and their SCHED and LOG forms: the kernels and the launcher of one form (the
                    # step loop they share, mdpp_grid_learn_body.inc, is listed in HEADERS)
                    **{u: ["mdpp_grid_learn.hpp"] for u in SOURCES if u.startswith("mdpp_grid_") and u.endswith("_learn.hip")},
                    # the closed-loop continuous units: the step and the history-2 act; the _summary and _h2 units include their family's .hip
                    **{f"mdpp_continuous_{pre}{fam}{suf}.hip": ([f"mdpp_continuous_{fam}.hip"] if pre or suf else []) + _CLOSED_DEPS
                       for fam in ("linear", "search", "es") for pre in ("", "summary_") for suf in ("", "_h2")}}
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off",
         "-fno-fast-math", "-Wall", "-Wno-unused-function"]
# The GENERAL kernels keep whole state vectors in registers and spill (k_continuous_step<DMAX=32, OMAX=4>: 3 KB of scratch per lane).
# With the compiler's default, SGPRs are spilled into the lanes of a VGPR, and where that VGPR is itself spilled inside divergent control
# flow the values parked in the inactive lanes are lost: k_continuous_step<32, 4, PHILOX> ended episodes that had not ended (lanes 43-60
# of a wave, whenever another lane of the wave ran the in-step reset; round 6, found by the random configurations against the oracle,
# pinned by tests/test_gpu_sweep.py::test_general_continuous_kernel_beyond_12_dimensions_on_philox_streams_vs_oracle).  These translation units spill SGPRs to memory instead; the hand-tuned rollout kernels do not spill and keep
# the default.
SPILL_SAFE = ["-mllvm", "-amdgpu-spill-sgpr-to-vgpr=0"]
# (+ the quiet kernel's two units: their Philox instantiations have 32 B of VGPR scratch and the flag costs them 0.4-1.5 %)
EXTRA_FLAGS = {s: SPILL_SAFE for s in ("mdpp_continuous.hip", "mdpp_continuous_line8.hip", "mdpp_discrete.hip", "mdpp_discrete_wide.hip",
                                       "mdpp_discrete_long.hip", "mdpp_discrete_quiet.hip", "mdpp_discrete_quiet_nu.hip")}
# (mdpp_continuous_linear.hip, mdpp_continuous_summary_linear.hip keep the default: their kernels spill SGPRs but no VGPR -- none is exposed by the rule of
#  tests/spill_exposed.py, whose pinned list of flagged units tests/test_kernel_spills.py holds this table to;
#  profiles/linear_rollout_resources.txt has every instantiation, tests/test_gpu_linear_rollout.py runs every lane against a twin;
#  mdpp_continuous_search.hip, mdpp_continuous_summary_search.hip likewise: profiles/linear_search_resources.txt, tests/test_gpu_linear_search.py;
#  mdpp_continuous_es.hip, mdpp_continuous_summary_es.hip likewise: profiles/linear_es_resources.txt, tests/test_gpu_linear_es.py;
#  the six *_h2.hip units -- the same kernels under a policy with memory -- likewise: profiles/linear_history_resources.txt,
#  tests/test_gpu_linear_history.py, tests/test_gpu_linear_history_search.py;
#  the six mdpp_discrete_trace*.hip / mdpp_discrete_summary_trace*.hip units likewise: profiles/learn_traces_resources.txt, tests/test_gpu_learn_traces.py;
#  the four mdpp_discrete_lambda_pe_pm*.hip / mdpp_discrete_summary_lambda_pe_pm*.hip units -- the trace kernels on one MDP per env -- likewise:
#  profiles/trace_seeds_resources.txt, tests/test_gpu_trace_seeds.py;
#  mdpp_grid_learn.hip, mdpp_grid_summary_learn.hip likewise: profiles/grid_learn_resources.txt, tests/test_gpu_grid_learn.py runs every lane against a twin;
#  the four mdpp_grid_*sched_learn.hip / mdpp_grid_episodes*_learn.hip units -- the same step loop with a schedule and / or an episode log -- likewise:
#  profiles/grid_schedule_resources.txt, tests/test_gpu_grid_schedule.py;
#  the six mdpp_grid_*levels*_learn.hip units -- the same six forms with per-env noise levels -- likewise:
#  profiles/grid_noise_levels_resources.txt, tests/test_gpu_grid_noise_levels.py)


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def _stale(target, deps, cmd=None):
    """True if target is missing, older than a dep, or (cmd given) was not built by exactly cmd: the command is kept
    beside the object in target + ".cmd", so a change of flags (EXTRA_FLAGS: SPILL_SAFE is a correctness flag)
    rebuilds the object without --force."""
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    if any(os.path.getmtime(d) > t for d in deps):
        return True
    return cmd is not None and _stamp(target) != _cmd_text(cmd)


def _cmd_text(cmd):
    return " ".join(cmd) + "\n"


def _stamp(target):
    try:
        with open(target + ".cmd") as f:
            return f.read()
    except OSError:
        return None


def _write_stamp(target, cmd):
    with open(target + ".cmd", "w") as f:
        f.write(_cmd_text(cmd))


def build(force=False, verbose=False):
    hipcc = _hipcc()
    srcs = [s for s in SOURCES if os.path.exists(os.path.join(CSRC, s))]
    hdrs = [os.path.join(CSRC, h) for h in HEADERS]
    objs, jobs = [], []
    for s in srcs:
        src = os.path.join(CSRC, s)
        obj = os.path.join(CSRC, s.replace(".hip", ".o"))
        objs.append(obj)
        extra = [os.path.join(CSRC, d) for d in INCLUDED_SOURCES.get(s, []) if os.path.exists(os.path.join(CSRC, d))]   # (like srcs: a missing one is hipcc's to report)
        cmd = [hipcc] + FLAGS + EXTRA_FLAGS.get(s, []) + ["-c", src, "-o", obj]
        if force or _stale(obj, [src] + extra + hdrs, cmd):
            jobs.append(cmd)

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        out = cmd[cmd.index("-o") + 1]
        if os.path.exists(out + ".cmd"):
            os.remove(out + ".cmd")    # a failed or interrupted compile leaves no stamp behind
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + " ".join(cmd) + "\n" + r.stdout)
        _write_stamp(out, cmd)
        return r.stdout

    if jobs:
        # the long compiles first (template-heavy kernels: 1.5-3 min each), as many at once as there are cores to spare
        heavy = ("mdpp_continuous_fast", "mdpp_discrete_lean", "mdpp_discrete_quiet", "mdpp_grid", "mdpp_continuous.", "mdpp_continuous_step1", "mdpp_continuous_linear", "mdpp_continuous_summary_linear",
                 "mdpp_continuous_search", "mdpp_continuous_summary_search", "mdpp_continuous_es", "mdpp_continuous_summary_es")
        jobs.sort(key=lambda c: next((k for k, h in enumerate(heavy) if h in c[-3]), len(heavy)))
        with ThreadPoolExecutor(max_workers=max(1, min(len(jobs), (os.cpu_count() or 4) - 1, 7))) as ex:
            for out in ex.map(run, jobs):
                if verbose and out.strip():
                    print(out)
    link = [hipcc, "--offload-arch=gfx950", "-shared", "-o", OUT] + objs
    if jobs or force or _stale(OUT, objs, link):
        run(link)
    return OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
