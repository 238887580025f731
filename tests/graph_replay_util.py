"""Test-side capture of ANY launch of a handle into a HIP graph, by the protocol of include/mdpp.h (the graph section) and of
RLToyVectorEnv.step_graph: read the step counter, switch the handle to capture mode, capture the call on a side stream, leave
capture mode, take the counter back.  replay() writes (counter now - counter at capture) to the handle's device word on the
current stream, launches the graph there and advances the counter by the call's steps.

Not a public API: the library's own graph entry point is step_graph (single steps).  The caller makes one eager launch of
the same call on the same handle BEFORE capture() -- what a first launch sets up (a kernel's LDS attribute, fills of parameter
arrays) then happens outside the capture -- and never captures a call that can fail: a failed capture's graph object aborts
the process when it is destroyed (see the comment in step_graph)."""
import ctypes as C
import gc

import torch

# Development switch (the sensitivity check of the cases; never set by a test): a replay writes offset 0 although the counter
# has moved.  A comparison that still passes does not test what it claims.
WITHHOLD_OFFSET = False


def tick(env):
    t = C.c_uint64()
    rc = env._lib.mdpp_tick(env._h, 0, C.byref(t))
    assert rc == 0, rc
    return int(t.value)


class CapturedCall:
    """capture(env, call, K): ``call()`` makes launches of K steps in all on ``env`` (env.rollout(acts, out),
    env.rollout_policy(K, out), env.rollout_learn(K, summary=s), ...) with every buffer it touches allocated beforehand."""

    def __init__(self, env, graph, K, tick0):
        self.env, self.graph, self.K, self.tick0 = env, graph, K, tick0

    def replay(self):
        env = self.env
        from mdp_playground_amd import _capi as capi
        off = 0 if WITHHOLD_OFFSET else tick(env) - self.tick0
        stream = C.c_void_p(torch.cuda.current_stream(env.device).cuda_stream)
        capi.check(env._lib, env._h, env._lib.mdpp_graph_set_tick_offset(env._h, off, stream), "mdpp_graph_set_tick_offset")
        self.graph.replay()
        capi.check(env._lib, env._h, env._lib.mdpp_tick(env._h, self.K, None), "mdpp_tick")


def capture(env, call, K):
    from mdp_playground_amd import _capi as capi
    lib, h = env._lib, env._h
    t0 = tick(env)
    side = torch.cuda.Stream(device=env.device)
    side.wait_stream(torch.cuda.current_stream(env.device))
    g = torch.cuda.CUDAGraph()
    capi.check(lib, h, lib.mdpp_graph_capture(h, 1), "mdpp_graph_capture")
    # No garbage collection while the capture is open: the finaliser of a handle an earlier, FAILED test left behind
    # (RLToyVectorEnv.__del__: a device synchronisation and hipFree) would run inside the capture, invalidate it, and the
    # failed graph's destructor aborts the process -- one failing case would take the whole session down.
    gc.collect()
    gc_was_on = gc.isenabled()
    gc.disable()
    try:
        # (thread-local capture, as in step_graph: a HIP call from another thread of the process must not invalidate it)
        with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
            call()
    finally:
        if gc_was_on:
            gc.enable()
        lib.mdpp_graph_capture(h, 0)
        lib.mdpp_tick(h, t0 - tick(env), None)          # the capture advanced the counter although nothing ran
    assert tick(env) == t0
    return CapturedCall(env, g, K, t0)
