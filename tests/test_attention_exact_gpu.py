"""The attention kernels against the structured probes of tests/attn_probes.py, whose float64
answers pin the weight of every single key: paged decode over its three merge routes, cascade
decode, paged causal prefill, the dense encoder, and the partial mode with ``q_past``.
tests/test_attn_probes_cpu.py shows what these comparisons reject."""
import functools
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_probes as P  # noqa: E402

from llm_kubernetes_minikube_sharp4dev_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
HKV = 2
ROUTES = ("reduce kernel", "fused merge", "partials")


@functools.lru_cache(maxsize=2)
def _decode_problem(kind, G, D, BS, split, prefix_blocks=None, extra_width=0):
    """Device tensors of one decode batch and its float64 answer; prefix_blocks: a cascade."""
    if prefix_blocks is None:
        ctx, k0 = P.DECODE_CTX, 0
    else:
        ctx, k0 = [prefix_blocks * BS + t for t in P.CASCADE_TAILS], prefix_blocks * BS
    probe = P.build(kind, P.decode_geom(ctx), HKV, G, D, split=split, BS=BS, k_start=k0)
    kc, vc, bt, cl = P.to_paged(probe, BS, extra_width=extra_width, shared_blocks=prefix_blocks or 0)
    q = torch.cat(probe.q)  # [B, Hq, D]
    return probe, q.to(DEV), kc.to(DEV), vc.to(DEV), bt.to(DEV), cl.to(DEV), probe.want_all()


def _merge_partials(y, part_o, part_ml, cl, k0, split, prefix):
    """The flash-decoding merge in float64 from the kernel's partials: part_ml = (max of the scores in
    log2 units, sum of 2^(score - max)), part_o = sum of 2^(score - max) v, per (row, head, split).  A
    row of one split and no prefix has no partials: the kernel wrote its output."""
    B, Hq, ms, D = part_o.shape
    out = y.double().cpu()
    po, pml = part_o.double().cpu(), part_ml.double().cpu()
    for b in range(B):
        ns = min(max(0, -(-(int(cl[b]) - k0) // split)), ms)
        if ns <= 1 and prefix is None:
            continue
        m = [pml[b, :, s, 0] for s in range(ns)]
        l = [pml[b, :, s, 1] for s in range(ns)]
        o = [po[b, :, s] for s in range(ns)]
        if prefix is not None:
            m.append(prefix[1][b, :, 0].double().cpu()), l.append(prefix[1][b, :, 1].double().cpu())
            o.append(prefix[0][b].double().cpu())
        M = torch.stack(m).amax(dim=0)
        f = [torch.where(torch.isinf(mi), torch.zeros_like(mi), torch.exp2(mi - M)) for mi in m]
        den = sum(fi * li for fi, li in zip(f, l))
        out[b] = sum(fi[:, None] * oi for fi, oi in zip(f, o)) / den[:, None]
    return out


def _decode(hip, problem, BS, split, route, k0=None, prefix=None, out=None):
    probe, q, kc, vc, bt, cl, _ = problem
    ms = ops.decode_splits(bt.shape[1] * BS, split)
    pp_o, pp_ml = prefix if prefix is not None else (None, None)
    if route == "reduce kernel":
        return hip.paged_decode(q, kc, vc, bt, cl, ms, split, probe.scale, None, None, out, k0, pp_o, pp_ml)
    if route == "fused merge":
        tickets = torch.zeros(q.shape[0] * HKV, dtype=torch.int32, device=DEV)
        ys = []
        for _ in range(2):  # the second launch starts from the tickets the first one left
            y = hip.paged_decode(q, kc, vc, bt, cl, ms, split, probe.scale, None, None, out, k0, pp_o, pp_ml, tickets)
            assert int(tickets.abs().sum()) == 0, "a ticket was not reset"
            ys.append(y.clone())
        assert torch.equal(ys[0], ys[1]), "the second fused launch differs from the first"
        return y
    B, Hq, D = q.shape
    part_o = torch.full((B, Hq, ms, D), float("nan"), device=DEV)
    part_ml = torch.full((B, Hq, ms, 2), float("nan"), device=DEV)
    y = hip.paged_decode(q, kc, vc, bt, cl, ms, split, probe.scale, part_o, part_ml,
                         torch.full_like(q, float("nan")), k0, pp_o, pp_ml, None, False)
    return _merge_partials(y, part_o, part_ml, cl.cpu(), int(k0[0]) if k0 is not None else 0, split, prefix)


def _decode_case(hip, kind, G, D, BS):
    for split in (128, 2048):
        problem = _decode_problem(kind, G, D, BS, split)
        for route in ROUTES:
            y = _decode(hip, problem, BS, split, route)
            P.check(kind, y.cpu(), problem[-1], f"decode {kind} G{G} D{D} BS{BS} split {split}, {route}, row")


@pytest.mark.parametrize("kind", ["U", "N", "W"])
@pytest.mark.parametrize("G", [1, 2, 4, 8])
@pytest.mark.parametrize("D", [64, 128])
def test_paged_decode_exact(hip, kind, G, D):
    _decode_case(hip, kind, G, D, 16)


@pytest.mark.parametrize("kind", ["U", "N", "W"])
@pytest.mark.parametrize("BS", [32, 128])
def test_paged_decode_exact_block_sizes(hip, kind, BS):
    _decode_case(hip, kind, 4, 128, BS)


@pytest.mark.parametrize("route", ROUTES[:2])
def test_paged_decode_strided_out(hip, route):
    """``out`` as a column slice of a wider tensor: rows strided, the columns beyond untouched."""
    problem = _decode_problem("W", 4, 128, 16, 128)
    q = problem[1]
    B, Hq, D = q.shape
    wide = torch.full((B, Hq * D + 64), 7.0, dtype=torch.bfloat16, device=DEV)
    out = wide[:, : Hq * D].view(B, Hq, D)
    y = _decode(hip, problem, 16, 128, route, out=out)
    assert y.data_ptr() == wide.data_ptr()
    P.check("W", wide[:, : Hq * D].reshape(B, Hq, D).cpu(), problem[-1], f"strided out, {route}")
    assert bool((wide[:, Hq * D:] == 7.0).all()), "columns beyond the slice were written"


@pytest.mark.parametrize("kind", ["U", "N"])
def test_paged_decode_wide_block_table(hip, kind):
    """A block table wider than any row needs (more splits launched than any row has), whose unused
    entries name a valid but wrong block."""
    for split in (128, 2048):
        problem = _decode_problem(kind, 4, 128, 16, split, None, 37)
        for route in ROUTES:
            y = _decode(hip, problem, 16, split, route)
            P.check(kind, y.cpu(), problem[-1], f"wide table {kind} split {split}, {route}")


@pytest.mark.parametrize("kind", ["U", "N", "W"])
@pytest.mark.parametrize("S", P.CASCADE_PREFIX_BLOCKS)
@pytest.mark.parametrize("G,D", [(1, 64), (4, 128), (8, 128), (2, 64)])
def test_cascade_decode_exact(hip, kind, S, G, D):
    """The first S blocks are shared by every row and attended once by the flash kernel in partial
    mode; the decode kernel attends the keys from k_start on and merges."""
    BS = 16
    for split in (128, 2048):
        problem = _decode_problem(kind, G, D, BS, split, S)
        probe, q, kc, vc, bt, cl, want = problem
        B, Hq = q.shape[0], q.shape[1]
        k0 = torch.tensor([S * BS], dtype=torch.int32, device=DEV)
        rpt = ops.prefill_rows_per_tile(G, D)
        nt = (B + rpt - 1) // rpt
        tiles = (torch.zeros(nt, dtype=torch.int32, device=DEV),
                 torch.arange(0, nt * rpt, rpt, dtype=torch.int32, device=DEV))
        pp_o = torch.full((B, Hq, D), float("nan"), device=DEV)
        pp_ml = torch.full((B, Hq, 2), float("nan"), device=DEV)
        cu = torch.tensor([0, B], dtype=torch.int32, device=DEV)
        ops.flash_prefill(q.view(B, Hq * D), kc, vc, cu, Hq, HKV, D, probe.scale, False, block_tables=bt[0:1],
                          ctx_lens=k0, tiles=tiles, part=(pp_o, pp_ml))
        for route in ROUTES:
            y = _decode(hip, problem, BS, split, route, k0, (pp_o, pp_ml))
            P.check(kind, y.cpu(), want, f"cascade {kind} G{G} D{D} prefix {S} blocks, split {split}, {route}, row")


def _prefill_problem(kind, geom, G, D, BS):
    probe = P.build(kind, geom, HKV, G, D, split=64, BS=BS)
    kc, vc, bt, cl = P.to_paged(probe, BS, seed=8)
    q = torch.cat(probe.q).reshape(-1, probe.Hq * D)
    q_lens = [probe.qlen(r) for r in range(probe.B)]
    cu = torch.tensor([0] + torch.tensor(q_lens).cumsum(0).tolist(), dtype=torch.int32)
    return probe, q.to(DEV), kc.to(DEV), vc.to(DEV), bt.to(DEV), cl.to(DEV), cu.to(DEV), q_lens


@pytest.mark.parametrize("kind", ["U", "N", "W"])
@pytest.mark.parametrize("G", [1, 2, 4, 8])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("BS", [8, 16, 128])
def test_flash_prefill_paged_exact(kind, G, D, BS):
    probe, q, kc, vc, bt, cl, cu, q_lens = _prefill_problem(kind, P.prefill_geom(P.PREFILL_QP), G, D, BS)
    y = ops.flash_prefill(q, kc, vc, cu, probe.Hq, HKV, D, probe.scale, True, block_tables=bt, ctx_lens=cl,
                          q_lens_cpu=q_lens, ctx_lens_cpu=cl.tolist())
    P.check(kind, y.cpu().view(-1, probe.Hq, D), probe.want_all(), f"prefill {kind} G{G} D{D} BS{BS}, query row")


@pytest.mark.parametrize("kind", ["U", "N", "W"])
@pytest.mark.parametrize("BS", [8, 16])
def test_flash_prefill_long_block_table(kind, BS):
    """Sequences of more than 128 cache blocks: the kernel holds the first 128 block-table entries of
    a sequence in registers and reads the later ones from memory."""
    G, D = 4, 128
    probe, q, kc, vc, bt, cl, cu, q_lens = _prefill_problem(kind, P.prefill_geom(P.LONG_QP), G, D, BS)
    assert bt.shape[1] > 128
    y = ops.flash_prefill(q, kc, vc, cu, probe.Hq, HKV, D, probe.scale, True, block_tables=bt, ctx_lens=cl,
                          q_lens_cpu=q_lens, ctx_lens_cpu=cl.tolist())
    P.check(kind, y.cpu().view(-1, probe.Hq, D), probe.want_all(), f"long prefill {kind} BS{BS}, query row")


@pytest.mark.parametrize("G", [1, 4])
def test_flash_prefill_staircase(G):
    """Tile maxima that walk around the threshold of the deferred running max: steps under it from
    the neighbouring tile but over it from the stale maximum, steps just over it, a fall of 30 and
    a climb of 20 log2 units; query rows that see from 1 key to all 13 tiles."""
    probe, q, kc, vc, bt, cl, cu, q_lens = _prefill_problem("S", P.prefill_geom(P.STAIR_QP), G, 128, 16)
    y = ops.flash_prefill(q, kc, vc, cu, probe.Hq, HKV, 128, probe.scale, True, block_tables=bt, ctx_lens=cl,
                          q_lens_cpu=q_lens, ctx_lens_cpu=cl.tolist())
    P.check("S", y.cpu().view(-1, probe.Hq, 128), probe.want_all(), f"staircase G{G}, query row")


@pytest.mark.parametrize("kind", ["U", "N"])
@pytest.mark.parametrize("D", [32, 64, 128])
def test_flash_encoder_dense_exact(kind, D):
    H = 4
    probe = P.build(kind, [(n, n, 0) for n in P.ENCODER_LENS], H, 1, D, causal=False)
    T = sum(P.ENCODER_LENS)
    qkv = torch.zeros(T, 3 * H * D, dtype=torch.bfloat16)
    qkv[:, : H * D] = torch.cat(probe.q).reshape(T, H * D)
    qkv[:, H * D: 2 * H * D] = torch.cat(probe.k).reshape(T, H * D)
    qkv[:, 2 * H * D:] = torch.cat(probe.v).reshape(T, H * D)
    qkv = qkv.to(DEV)
    cu = torch.tensor([0] + torch.tensor(P.ENCODER_LENS).cumsum(0).tolist(), dtype=torch.int32, device=DEV)
    y = ops.flash_prefill(qkv[:, : H * D], qkv[:, H * D: 2 * H * D], qkv[:, 2 * H * D:], cu, H, H, D, probe.scale,
                          False, q_lens_cpu=P.ENCODER_LENS)
    P.check(kind, y.cpu().view(T, H, D), probe.want_all(), f"encoder {kind} D{D}, row")


@pytest.mark.parametrize("kind", ["U", "W"])
def test_flash_prefill_partials_q_past(kind):
    """Partial mode over the key shard of a context-parallel rank: q_past negative for part of the
    rows, zero, inside the keys and past all keys.  Rows that see no key return l == 0; the others
    o / l against the float64 answer and m + log2(l) against the float64 log-sum-exp.

    Tolerance of m + log2(l): l sums n <= 300 terms 2^(s - m) in f32.  A term is off by at most
    2^-23 (the exp2 instruction, 1 ulp) + ln 2 * 2^-21 (its argument, |s| <= 8 log2 units, rounded
    in f32) relative, the sum by n * 2^-24 relative, m by 8 * 2^-24: together less than
    log2(e) * (n + 16) * 2^-24 + 2^-20 = 2.8e-5 at n = 300."""
    G, D = 4, 128
    probe, q, kc, vc, bt, cl, cu, q_lens = _prefill_problem(kind, P.SHARD_GEOM, G, D, 16)
    qp = torch.tensor(probe.past, dtype=torch.int32, device=DEV)
    T = q.shape[0]
    po = torch.full((T, probe.Hq, D), float("nan"), device=DEV)
    pml = torch.full((T, probe.Hq, 2), float("nan"), device=DEV)
    ops.flash_prefill(q, kc, vc, cu, probe.Hq, HKV, D, probe.scale, True, block_tables=bt, ctx_lens=cl,
                      q_lens_cpu=q_lens, ctx_lens_cpu=cl.tolist(), part=(po, pml), q_past=qp)
    po, m, l = po.cpu().double(), pml[..., 0].cpu().double(), pml[..., 1].cpu().double()
    want = probe.want_all()
    lse2 = torch.cat([probe.lse2(r) for r in range(probe.B)])
    blind = torch.isinf(lse2)
    assert bool(blind.any()) and bool((~blind).any())
    assert bool((l[blind] == 0).all()), "a row without a visible key has l != 0"
    assert bool((l[~blind] > 0).all())
    got = torch.where(blind[..., None], torch.zeros_like(po), po / l.clamp_min(1e-300)[..., None])
    P.check(kind, got, want, f"partials {kind}, query row")
    n = max(g[0] for g in P.SHARD_GEOM)
    tol = P.LOG2E * (n + 16) * 2.0 ** -24 + 2.0 ** -20
    err = ((m + torch.log2(l))[~blind] - lse2[~blind]).abs().max()
    print(f"partials {kind}: |m + log2 l - lse| max {float(err):.3g} (tolerance {tol:.3g})")
    assert float(err) <= tol


def test_launchers_reject_unsupported_shapes(hip):
    """Shapes the launchers are documented to reject raise before anything is launched: ``out``
    keeps its sentinel."""
    bf = dict(dtype=torch.bfloat16, device=DEV)
    i32 = dict(dtype=torch.int32, device=DEV)

    def decode(Hq, D, BS, split):
        q = torch.zeros(2, Hq, D, **bf)
        kc = torch.zeros(4, HKV, BS, D, **bf)
        out = torch.full_like(q, 7.0)
        with pytest.raises(RuntimeError):
            hip.paged_decode(q, kc, kc.clone(), torch.zeros(2, 2, **i32), torch.ones(2, **i32), 1, split,
                             1 / math.sqrt(D), None, None, out)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())

    decode(8, 128, 48, 128)   # a block size that does not divide the split
    decode(8, 128, 24, 96)    # a block size that is no multiple of 16
    decode(6, 128, 16, 128)   # GQA group 3
    decode(32, 128, 16, 128)  # GQA group 16
    decode(8, 32, 16, 128)    # head dim 32
    decode(8, 128, 16, 4096)  # a split beyond the workgroup's block-table slice

    def prefill(Hq, D, BS):
        q = torch.zeros(5, Hq * D, **bf)
        kc = torch.zeros(4, HKV, BS, D, **bf)
        out = torch.full_like(q, 7.0)
        tiles = (torch.zeros(1, **i32), torch.zeros(1, **i32))
        with pytest.raises(RuntimeError):
            ops.flash_prefill(q, kc, kc.clone(), torch.tensor([0, 5], **i32), Hq, HKV, D, 1 / math.sqrt(D), True,
                              block_tables=torch.zeros(1, 4, **i32), ctx_lens=torch.tensor([5], **i32), tiles=tiles,
                              out=out)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())

    prefill(6, 128, 16)   # GQA group 3
    prefill(8, 128, 24)   # a cache block that is no power of two
    prefill(8, 128, 2)    # a cache block smaller than the rows one wave stages
    prefill(8, 256, 16)   # head dim 256


def test_probes_reject_a_decode_context_one_key_short(hip):
    """The comparison can fail on the GPU: with every context length one too small (the last key
    dropped) each row of two or more keys is rejected by at least one of U, N and W; the one-key
    row, left as it was, still passes."""
    for route in ROUTES[:2]:
        worst = torch.zeros(len(P.DECODE_CTX), dtype=torch.float64)
        for kind in "UNW":
            probe, q, kc, vc, bt, cl, want = _decode_problem(kind, 4, 128, 16, 128)
            short = (probe, q, kc, vc, bt, (cl - 1).clamp(min=1), want)
            x = P.excess(kind, _decode(hip, short, 16, 128, route).cpu(), want).flatten(1).amax(dim=1)
            for r in range(probe.B):
                worst[probe.seq[r]] = max(worst[probe.seq[r]], x[r])
        for s, n in enumerate(P.DECODE_CTX):
            assert (worst[s] > 1) == (n > 1), f"{n} keys, {route}: {float(worst[s]):.3g} x tolerance"


def test_probes_reject_a_causal_mask_one_key_short():
    """The same for prefill: with q_past one too small every query row loses its last visible key,
    and every row is rejected by at least one of U, N and W."""
    G, D = 4, 128
    worst = None
    for kind in "UNW":
        probe, q, kc, vc, bt, cl, cu, q_lens = _prefill_problem(kind, P.prefill_geom(P.PREFILL_QP), G, D, 16)
        qp = torch.tensor(probe.past, dtype=torch.int32, device=DEV) - 1
        y = ops.flash_prefill(q, kc, vc, cu, probe.Hq, HKV, D, probe.scale, True, block_tables=bt, ctx_lens=cl,
                              q_lens_cpu=q_lens, ctx_lens_cpu=cl.tolist(), q_past=qp)
        x = P.excess(kind, y.cpu().view(-1, probe.Hq, D), probe.want_all()).flatten(1).amax(dim=1)
        worst = x if worst is None else torch.maximum(worst, x)
    assert bool((worst > 1).all()), f"query rows {torch.nonzero(worst <= 1).flatten().tolist()} pass every probe"
