"""The engine probes of tests/engine_probes.py on the GPU: the scenarios of its module docstring through
the real LLMEngine, Scheduler, allocator and ModelRunner over the HIP kernels, with hipGraphs on and
off, ``step()`` and ``step_pipelined()``, probes U and N.  The KV cache starts as NaN; every row the
scheduler ran is checked against the float64 answer of the (sequence, position) its id names, every
request's tokens against its script, and after every collect the cache slots of every running
sequence, and of every block just published to the prefix cache, against its K / V bit for bit.
tests/test_engine_probes_cpu.py shows what these checks reject and pins the schedule
(``engine_probes.STEPS``) that the runs here must repeat."""
import functools
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import engine_probes as EP  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCENARIOS = ["A", "A64", "B", "C", "C-nocache", "D", "D-tight", "E"]


@functools.lru_cache(maxsize=None)
def spec(name, kind):
    """One scene, and its float64 answers, for the four runs of a (scenario, probe)."""
    return EP.SPECS[name](kind)


@pytest.mark.parametrize("pipelined", [False, True], ids=["step", "pipelined"])
@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graphs"])
@pytest.mark.parametrize("kind", ["U", "N"])
@pytest.mark.parametrize("name", SCENARIOS)
def test_scenario(name, kind, graphs, pipelined):
    t0 = time.perf_counter()
    h = EP.Harness(spec(name, kind), DEV, graphs=graphs, pipelined=pipelined)
    assert h.runner.use_graphs == graphs and h.runner.kv.is_cuda and bool(torch.isnan(h.runner.kv).all())
    st = h.run()
    torch.cuda.synchronize()
    print(f"\n{name} {kind} {'graphs' if graphs else 'eager'} {'pipelined' if pipelined else 'step'}: "
          f"{time.perf_counter() - t0:.2f} s, {({k: v for k, v in st.items() if v})}")
    assert st["steps"] == EP.STEPS[name][pipelined], "the schedule is not the CPU run's"
    assert st["steps"] == st["replays"] + st["eager"]
    if pipelined:
        assert st["gathers"] > 0, "no step gathered in-flight ids on the device"
    else:
        assert st["gathers"] == 0
    if graphs:
        assert st["replays"] > 0, "no bucket was replayed"
        assert st["mixed"] > 0 and st["eager"] > 0, "no eager mixed step"
        assert len(h.runner.graphs) > 1
    else:
        assert st["replays"] == 0 and not h.runner.graphs
