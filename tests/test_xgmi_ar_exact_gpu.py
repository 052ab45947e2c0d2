"""The xGMI collectives (csrc/xgmi_allreduce.hip, K14) against the probes of tests/ar_probes.py, which
pin per element the ranks that were read, the order they were added in and the roundings: every
all-reduce form (one-shot, two-shot, all_reduce_ under both forced settings, the fused residual +
RMSNorm forms and their reduce loops), the gather kernel and the chunked wrapper path, bit for bit
(only the fused forms' normalised output under row_probes' "rms" limit).  Every result is the
leading part of a SENTINEL-filled buffer whose tail must stay untouched, and no input is written.

The ranks are processes on device 0 (as tests/test_xgmi_ar_gpu.py); ONE spawn per world runs every
probe of that world on one XgmiAllReduce object, so the kernel forms share the per-workgroup epochs
throughout.  Each rank saves (name, ok, first bad index, got, want) rows; the parent asserts them.
tests/test_ar_probes_cpu.py shows what these comparisons reject.

Wall time on an MI355X, measured in one session: this file 12.8 s (2.5 / 3.6 / 4.7 s for world
2 / 3 / 8, three spawns); tests/test_xgmi_ar_gpu.py 37.6 s before its data became the layout probe's
and 38.6 s after (nine spawns)."""
import os
import sys
import tempfile
import time

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ar_probes as A  # noqa: E402
import row_probes as R  # noqa: E402
from test_xgmi_ar_gpu import _free_port  # noqa: E402  (also caps LK_XGMI_AR_BLOCKS at 32)

pytestmark = pytest.mark.gpu
os.environ.setdefault("LK_XGMI_AR_BLOCKS", str(A.BLOCKS))
BF = torch.bfloat16
EPS = R.NORM_EPS
DEV = "cuda"
MID = 8 * 513


class _Stop(Exception):
    """A handshake timed out (the error word is set): this rank issues no further collective."""


class _Run:
    def __init__(self, rank, world, ars):
        self.rank, self.world, self.ars, self.rows = rank, world, ars, []

    def go(self):
        """Before every collective: stop for good once an error word is set."""
        for ar in self.ars:
            e = ar.error()
            if e:
                self.rows.append((f"error word {e} before collective {len(self.rows)}", False, -1, float(e), 0.0))
                raise _Stop

    def check(self, name, got, want, kind="E"):
        torch.cuda.synchronize()
        self.rows.append(A.verdict(name, got, want, kind))

    def unchanged(self, name, t, keep):
        self.check(name + ": the input is not written", t, keep)


def _guarded_copy(x, guard=A.GUARD):
    buf, view = A.guarded(x.numel(), DEV, guard)
    view.copy_(x.reshape(-1))
    return buf, view


# ---------------------------------------------------------------- 1. reduce probes
def _reduce_probes(run, ar):
    world, rank = run.world, run.rank
    probes = [(f"layout n{n}", A.layout(world, n, seed=n)) for n in A.PLAIN_N]
    probes.append((f"rounding n{MID}", A.rounding(world, MID)[:2]))
    if world >= 3:
        probes.append((f"order n{MID}", A.order(world, MID)))
    for name, (xs, want) in probes:
        n = want.numel()
        x = xs[rank].to(DEV)
        keep = x.clone()
        # one-shot, out of place and in place
        run.go()
        buf, view = A.guarded(n, DEV)
        ar.state.all_reduce(x, view)
        run.check(f"{name} all_reduce", buf, want)
        run.unchanged(f"{name} all_reduce", x, keep)
        run.go()
        buf, view = _guarded_copy(x)
        ar.state.all_reduce(view, view)
        run.check(f"{name} all_reduce in place", buf, want)
        # two-shot, a 1-D message as rows of 8 (one active lane per row)
        run.go()
        buf, view = A.guarded(n, DEV)
        ar.state.all_reduce2(x.view(-1, 8), view.view(-1, 8))
        run.check(f"{name} all_reduce2 rows of 8", buf, want)
        run.unchanged(f"{name} all_reduce2", x, keep)
        run.go()
        buf, view = _guarded_copy(x)
        ar.state.all_reduce2(view.view(-1, 8), view.view(-1, 8))
        run.check(f"{name} all_reduce2 rows of 8 in place", buf, want)
        # the wrapper under both forced settings
        for forced in (True, False):
            run.go()
            buf, view = _guarded_copy(x)
            ar.two_shot = forced
            try:
                assert ar.eligible(view)
                ar.all_reduce_(view)
            finally:
                ar.two_shot = None
            run.check(f"{name} all_reduce_ two_shot={forced}", buf, want)
    # two-shot owner slices: rows below, at and above the world size, short and empty owners,
    # more rows per owner than workgroups
    H = A.FUSED_H
    for T in A.two_shot_T(world):
        xs, want = A.layout(world, T * H, seed=1000 + T)
        x = xs[rank].to(DEV).view(T, H)
        keep = x.clone()
        run.go()
        buf, view = A.guarded(T * H, DEV)
        ar.state.all_reduce2(x, view.view(T, H))
        run.check(f"layout all_reduce2 T{T} H{H}", buf, want)
        run.unchanged(f"layout all_reduce2 T{T} H{H}", x, keep)
        run.go()
        buf, view = _guarded_copy(x)
        ar.state.all_reduce2(view.view(T, H), view.view(T, H))
        run.check(f"layout all_reduce2 T{T} H{H} in place", buf, want)


# ---------------------------------------------------------------- 2. fused probes
def _fused_call(run, ar, algo, x, res, w, T, H):
    """-> (residual buffer, out buffer), [T + 1, H] each with a SENTINEL last row."""
    run.go()
    rbuf, rview = _guarded_copy(res, H)
    obuf, oview = A.guarded(T * H, DEV, H)
    out = ar.all_reduce_rmsnorm_(x, rview.view(T, H), w, EPS, out=oview.view(T, H), algo=algo)
    assert out.data_ptr() == obuf.data_ptr()
    return rbuf, obuf


def _fused_shapes(world):
    shapes = [(A.FUSED_H, T) for T in sorted(set(A.FUSED_T) | set(A.two_shot_T(world)))]
    for H in R.NORM_H:
        shapes += [(H, T) for T in sorted({A.WIDE_T, world + 1})]
    return shapes


def _fused_probes(run, ar):
    from llm_kubernetes_minikube_sharp4dev_amd import ops

    world, rank = run.world, run.rank
    for H, T in _fused_shapes(world):
        f = A.fused(world, H, T)
        x, w = f["xs"][rank].to(DEV), f["w"].to(DEV)
        keep = x.clone()
        got = {}
        for algo in ("ipc1", "ipc2"):
            name = f"fused H{H} T{T} {algo}"
            rbuf, obuf = _fused_call(run, ar, algo, x, f["res"].to(DEV), w, T, H)
            run.check(f"{name} residual", rbuf, f["want_res"])
            run.check(f"{name} out", obuf, f["want_out"], "rms")
            run.unchanged(name, x, keep)
            got[algo] = (rbuf, obuf)
        run.check(f"fused H{H} T{T} out ipc2 == ipc1", got["ipc2"][1], got["ipc1"][1][: T * H])
        # the unfused chain on the bf16 sum: the add + norm kernel, bit for bit
        ref_r = f["res"].to(DEV)
        ref_y = ops.rmsnorm(f["sum"].to(DEV), w, EPS, residual=ref_r)
        run.check(f"fused H{H} T{T} out == ops.rmsnorm(sum, residual)", got["ipc1"][1], ref_y)
        run.check(f"fused H{H} T{T} residual == ops.rmsnorm's", got["ipc1"][0], ref_r)
    # the fused kernels' own reduce loops under the order and rounding probes: with a zero residual
    # the new residual is bf16(bf16(sum) + 0), the all-reduce's bits (rows of NaN normalise to NaN:
    # the output is not compared)
    T, H = 33, A.FUSED_H
    probes = [("layout", A.layout(world, T * H, seed=5)), ("rounding", A.rounding(world, T * H)[:2])]
    if world >= 3:
        probes.append(("order", A.order(world, T * H)))
    w = torch.ones(H, dtype=BF, device=DEV)
    zero = torch.zeros(T, H, dtype=BF, device=DEV)
    for name, (xs, want) in probes:
        x = xs[rank].to(DEV).view(T, H)
        for algo in ("ipc1", "ipc2"):
            rbuf, _ = _fused_call(run, ar, algo, x, zero, w, T, H)
            run.check(f"{name} through the fused {algo} reduce, residual", rbuf, want)


# ---------------------------------------------------------------- 4. shared epochs
def _shared_epochs(run, ar):
    """One object, kernel forms of 1 and 32 workgroups mixed: workgroup 0's epoch runs ahead of
    workgroup 31's and the two-shot phase-2 flags lag phases 0 / 1 by every one-shot call."""
    from llm_kubernetes_minikube_sharp4dev_amd import ops

    world, rank = run.world, run.rank
    H = A.FUSED_H
    w = torch.ones(H, dtype=BF, device=DEV)
    for rep in range(2):
        seed = 100 * (rep + 1)

        def data(n, step):
            xs, want = A.layout(world, n, seed=seed + step)
            return xs, xs[rank].to(DEV), want

        name = f"epochs pass {rep}"
        run.go()
        xs, x, want = data(8, 0)
        buf, view = A.guarded(8, DEV)
        ar.state.all_reduce(x, view)
        run.check(f"{name}: plain 8 elements", buf, want)
        for step, algo, T in ((1, "ipc2", 33 * world + 1), (2, "ipc1", 5)):
            xs, x, want = data(T * H, step)
            rbuf, obuf = _fused_call(run, ar, algo, x.view(T, H), torch.zeros(T, H, dtype=BF, device=DEV), w, T, H)
            run.check(f"{name}: fused {algo} T{T} residual", rbuf, want)
            ref_r = torch.zeros(T, H, dtype=BF, device=DEV)
            run.check(f"{name}: fused {algo} T{T} out", obuf, ops.rmsnorm(want.to(DEV).view(T, H), w, EPS, residual=ref_r))
        run.go()
        xs, x, want = data(20, 3)  # 40 bytes, padded to 48 by the wrapper
        got = ar.all_gather(x)
        run.check(f"{name}: all_gather of 40 bytes", got, torch.stack(xs))
        run.go()
        xs, x, want = data(MID, 4)
        buf, view = _guarded_copy(x)
        ar.broadcast_(view, root=world - 1)
        run.check(f"{name}: broadcast from the last rank", buf, xs[world - 1])
        run.go()
        xs, x, want = data(A.PLAIN_N[4], 5)
        buf, view = A.guarded(want.numel(), DEV)
        ar.state.all_reduce(x, view)
        run.check(f"{name}: plain {want.numel()} elements", buf, want)
        run.go()
        xs, x, want = data(H, 6)
        buf, view = A.guarded(H, DEV)
        ar.state.all_reduce2(x.view(1, H), view.view(1, H))
        run.check(f"{name}: two-shot plain T1", buf, want)


# ---------------------------------------------------------------- 5. gather
def _gather(run, ar):
    world, rank = run.world, run.rank
    for n in A.PLAIN_N:
        xs, _ = A.layout(world, n, seed=7 * n)
        x = xs[rank].to(DEV)
        keep = x.clone()
        run.go()
        buf, view = A.guarded(world * n, DEV)
        ar.state.gather(x, view, -1)
        run.check(f"all-gather n{n}", buf, torch.cat(xs))
        run.unchanged(f"all-gather n{n}", x, keep)
        for root in (0, world - 1):
            run.go()
            if rank == root:  # the root's out aliases its in
                buf, view = _guarded_copy(x)
                ar.state.gather(view, view, root)
            else:
                buf, view = A.guarded(n, DEV)
                ar.state.gather(x, view, root)
            run.check(f"broadcast n{n} from {root}", buf, xs[root])
            run.unchanged(f"broadcast n{n} from {root}", x, keep)


# ---------------------------------------------------------------- 6. the chunked wrapper path
def _chunked(run, small):
    """max_bytes 64 KiB = 32768 elements per chunk: sizes that are no multiple of 8, a view that is
    not contiguous and a slice whose data pointer is 2 bytes off the 16-byte alignment."""
    world, rank = run.world, run.rank
    n = 3 * 32768 + 13
    xs, want = A.layout(world, n, seed=11)
    run.go()
    buf, view = _guarded_copy(xs[rank].to(DEV))
    assert not small.eligible(view)
    small.all_reduce_(view)
    run.check(f"chunked n{n} (4 chunks)", buf, want)
    rows, cols = 40, 1024  # 40960 elements: 2 chunks
    xs, want = A.layout(world, rows * cols, seed=12)
    run.go()
    base = torch.full((rows, 2 * cols), A.SENTINEL, dtype=BF, device=DEV)
    view = base[:, ::2]
    view.copy_(xs[rank].to(DEV).view(rows, cols))
    assert not view.is_contiguous()
    small.all_reduce_(view)
    full = torch.full((rows, 2 * cols), A.SENTINEL, dtype=BF)
    full[:, ::2] = want.view(rows, cols)
    run.check("chunked [:, ::2] view, the odd columns untouched", base, full)
    n = 32768 + 40
    xs, want = A.layout(world, n, seed=13)
    run.go()
    base = torch.full((1 + n + A.GUARD,), A.SENTINEL, dtype=BF, device=DEV)
    view = base[1:1 + n]
    view.copy_(xs[rank].to(DEV))
    assert view.data_ptr() % 16 == 2 and not small.eligible(view)
    small.all_reduce_(view)
    run.check("chunked x[1:] slice, 2 bytes off alignment", base, torch.cat([torch.full((1,), A.SENTINEL, dtype=BF), want]))


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(2)  # up to 8 ranks build their probes side by side
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from llm_kubernetes_minikube_sharp4dev_amd.parallel.tp import TPGroup
    from llm_kubernetes_minikube_sharp4dev_amd.parallel.xgmi_ar import XgmiAllReduce

    tp = TPGroup(rank, world, dist.group.WORLD, ctrl=dist.group.WORLD, ranks=list(range(world)))
    ar = XgmiAllReduce(tp, 16 << 20)
    small = XgmiAllReduce(tp, 64 << 10)
    run = _Run(rank, world, (ar, small))
    sections = []
    try:
        for name, fn, obj in (("reduce", _reduce_probes, ar), ("fused", _fused_probes, ar), ("epochs", _shared_epochs, ar),
                              ("gather", _gather, ar), ("chunked", _chunked, small)):
            t0 = time.time()
            fn(run, obj)
            sections.append((name, len(run.rows), round(time.time() - t0, 1)))
        torch.cuda.synchronize()
        run.rows.append(("error() == 0 at the end", ar.error() == 0 and small.error() == 0, -1, float(ar.error()), 0.0))
    except _Stop:
        pass
    except Exception as e:  # a refused call on this rank: recorded; the peers stop at their next handshake
        run.rows.append((f"{type(e).__name__}: {e}"[:400], False, -1, 0.0, 0.0))
    torch.save({"rows": run.rows, "sections": sections}, os.path.join(out_dir, f"x{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", A.WORLDS)
def test_xgmi_collectives_exact(world):
    t0 = time.time()
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(world, _free_port(), d), nprocs=world, join=True)
        saved = [torch.load(os.path.join(d, f"x{r}.pt"), weights_only=True) for r in range(world)]
    print(f"world {world}: {len(saved[0]['rows'])} comparisons per rank, sections {saved[0]['sections']}, {time.time() - t0:.1f} s")
    bad = [(r, row) for r, s in enumerate(saved) for row in s["rows"] if not row[1]]
    for r, (name, _, idx, got, want) in bad[:10]:
        print(f"rank {r}: {name}: first wrong element {idx}: got {got!r}, want {want!r}")
    assert not bad, f"{len(bad)} comparisons failed; the first on rank {bad[0][0]}: {bad[0][1]}"
    assert len({len(s["rows"]) for s in saved}) == 1 and len(saved[0]["sections"]) == 5
    assert saved[0]["rows"][-1][0] == "error() == 0 at the end"
