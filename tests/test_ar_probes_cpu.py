"""tests/ar_probes.py without a GPU: the two references agree on every probe, the exact probes are
exact, and -- the point of the probes -- the emulation of each all-reduce form passes every probe
unmutated and fails the probe family designated for it with ONE injected fault, for each world in
2, 3, 8, under the comparison the GPU test uses (ar_probes.verdict).  Take a probe family away and
the tests of its mutants fail."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ar_probes as A  # noqa: E402
import row_probes as R  # noqa: E402

BF = torch.bfloat16
BIG = 8 * (32 * 512 + 1)  # 32 workgroups of 513 vectors
MID = 8 * 513             # 2 workgroups


def _ok(v):
    return v[1]


def _sum64(xs):
    return sum(x.double() for x in xs)


# ---------------------------------------------------------------- the comparison itself
def test_verdict_is_bitwise_and_guards_the_tail():
    want = torch.tensor([1.0, 0.0, float("nan"), float("inf")]).to(BF)
    buf, view = A.guarded(4)
    view.copy_(want)
    assert A.verdict("same", buf, want) == ("same", True, -1, 0.0, 0.0)
    for i, v in enumerate([1.0078125, -0.0, float("inf"), float("nan")]):
        b = buf.clone()
        b[i] = v
        name, ok, idx, _, _ = A.verdict("x", b, want)
        assert not ok and idx == i
    b = buf.clone()
    b[4 + A.GUARD - 1] = 0.0
    assert A.verdict("tail", b, want)[1:3] == (False, 4 + A.GUARD - 1)
    assert A.verdict("short", buf[:3], want)[1] is False
    w64 = torch.tensor([[1.0, 2.0, 3.0, 4.0]], dtype=torch.float64)
    near = torch.cat([torch.tensor([1.0, 2.0, 3.0, 4.03125]).to(BF), torch.full((4,), A.SENTINEL, dtype=BF)])
    assert _ok(A.verdict("rms", near, w64, "rms"))
    near[3] = 4.125
    assert not _ok(A.verdict("rms", near, w64, "rms"))


# ---------------------------------------------------------------- the references
@pytest.mark.parametrize("world", A.WORLDS)
def test_references_agree_and_exact_probes_are_exact(world):
    for n in A.PLAIN_N[:5]:
        xs, want = A.layout(world, n, seed=n)
        assert torch.equal(_sum64(xs), want.double()) and float(want.max()) <= 2 ** world - 1
        assert n == 8 or set(want.double().tolist()) == set(range(2 ** world)), "every subset of the ranks"
        assert not bool(A.mismatch(A.ref64(xs), want).any()) and not bool(A.mismatch(A.emu_allreduce(xs), want).any())
        # exact in any order and with a bf16 accumulator: the probe is about placement alone
        for rank in range(world):
            assert not bool(A.mismatch(A.emu_allreduce(xs, "rotate", rank), want).any())
        assert not bool(A.mismatch(A.emu_allreduce(xs, "bf16_acc"), want).any())
    # no period in the element index: no shift by a multiple of 8 up to 4096 + 8 maps a rank's data to itself
    xs, _ = A.layout(world, BIG)
    for r in range(world):
        for s in list(range(8, 4105, 8)) + [8 * 513, 8192]:
            assert not torch.equal(xs[r][s:], xs[r][:-s]), (r, s)
    # rank r's data does not depend on the world size, the seed changes it
    assert all(torch.equal(a, b) for a, b in zip(xs, A.layout(8, BIG)[0]))
    assert not torch.equal(xs[0], A.layout(world, BIG, seed=1)[0][0])
    xs, want, case = A.rounding(world, MID)
    assert not bool(A.mismatch(A.ref64(xs), want).any()) and not bool(A.mismatch(A.emu_allreduce(xs), want).any())
    ncase = int(case.max()) + 1
    assert ncase == (12 if world >= 3 else 10)
    assert bool(torch.isnan(want[case == 4]).all()) and bool(torch.isnan(want[case == 5]).all())
    z = want[case == ncase - 1]
    assert bool((A.bits(z) == 0).all()), "+0.0, not -0.0"
    assert all(bool((A.bits(x[case == ncase - 1]) == -32768).all()) for x in xs), "every rank gives -0.0"
    sub = want[(case >= 6) & (case <= 8)].double()
    assert sorted(set((sub / A.TINY).tolist())) == [8.0, 57.0, 200.0], "subnormal sums are kept"
    for H in (8, 520, 1024, 4104):
        for T in (1, 5):
            f = A.fused(world, H, T)
            assert torch.equal(_sum64(f["xs"])[~f["dbl"]], f["sum"].double()[~f["dbl"]])
            assert not bool(A.mismatch(A.ref64(f["xs"]), f["sum"]).any())
            for rank in range(world):  # every partial sum is exact in f32: any order gives the same bits
                assert not bool(A.mismatch(A.emu_allreduce(f["xs"], "rotate", rank), f["sum"]).any())
            if T > 1:
                assert bool((_sum64(f["xs"])[1].abs() == 257).all()) and bool((f["want_res"][1].double().abs() == 256).all())
                assert bool(((f["sum"][1].double() + f["res"][1].double()).abs() == 257).all())
            # the value's rank is spread over all ranks, the idle ranks give zero
            nz = torch.stack([x != 0 for x in f["xs"]]).sum(0)
            assert int(nz.max()) <= min(world, 4 if T > 1 else 3)
            if H >= 520:
                assert all(bool((x != 0).any()) for x in f["xs"])


@pytest.mark.parametrize("world", [3, 8])
def test_order_probe_pins_the_rank_order(world):
    """The f32 sum in rank order is +0; the float64 sum is 1 (which is why emu_allreduce, not ref64,
    is this probe's reference); started at any other rank the sum is 1 somewhere."""
    xs, want = A.order(world, MID)
    assert bool((_sum64(xs) == 1).all())
    got = A.emu_allreduce(xs)
    assert not bool(A.mismatch(got, want).any()) and bool((A.bits(got) == 0).all())
    assert not bool(A.mismatch(A.emu_allreduce(xs, "rotate", 0), want).any()), "rank 0 starts at itself"
    for rank in range(1, world):
        got = A.emu_allreduce(xs, "rotate", rank)
        # 1 where a < rank <= c, 0 elsewhere (world 3 has the one triple: 1 everywhere)
        assert set(got.double().unique().tolist()) == ({1.0} if world == 3 else {0.0, 1.0}), rank
    # every triple of ranks is there, and a reversed order gives 1 everywhere
    ntrip = world * (world - 1) * (world - 2) // 6
    pat = torch.stack([x[:ntrip].double() for x in xs])
    assert len({tuple(pat[:, i].tolist()) for i in range(ntrip)}) == ntrip
    assert bool((A.emu_allreduce(xs[::-1]).double() == 1).all())


# ---------------------------------------------------------------- sensitivity
def _plain(family, world, n=BIG, seed=2):
    if family == "layout":
        return A.layout(world, n, seed)
    if family == "order":
        return A.order(world, n)
    return A.rounding(world, n)[:2]


def _rejects_plain(family, world, mutant, two_shot=False):
    """Some rank's emulated result fails the probe."""
    T = 2 * world + 1
    xs, want = _plain(family, world, T * A.FUSED_H if two_shot else BIG)
    prev, _ = _plain(family, world, T * A.FUSED_H if two_shot else BIG, seed=1)
    bad = False
    for rank in range(world):
        if two_shot:
            v = [x.view(T, A.FUSED_H) for x in xs]
            buf = A.emu_allreduce2(v, mutant, rank, [p.view(T, A.FUSED_H) for p in prev])
        else:
            buf, view = A.guarded(xs[0].numel())
            view.copy_(A.emu_allreduce(xs, mutant, rank, prev))
        bad |= not _ok(A.verdict(f"{family} {mutant} rank {rank}", buf, want))
    return bad


def _rejects_fused(world, mutant, two_shot=False, H=A.FUSED_H, T=None):
    T = T or 2 * world + 1
    f, prev = A.fused(world, H, T), A.fused(world, H, T, seed=1)
    bad = False
    for rank in range(world):
        rbuf, obuf = A.emu_fused(f["xs"], f["res"], f["w"], mutant=mutant, rank=rank, prev=prev["xs"], two_shot=two_shot)
        bad |= not _ok(A.verdict("res", rbuf, f["want_res"]))
        bad |= not _ok(A.verdict("out", obuf, f["want_out"], "rms"))
    return bad


@pytest.mark.parametrize("world", A.WORLDS)
def test_unmutated_emulations_pass_every_probe(world):
    for family in ("layout", "rounding") + (("order",) if world >= 3 else ()):
        assert not _rejects_plain(family, world, None) and not _rejects_plain(family, world, None, True)
    for T in A.two_shot_T(world):
        assert not _rejects_fused(world, None, True, T=T)
        xs, want = A.layout(world, T * A.FUSED_H, seed=T)
        for rank in (0, world - 1):
            assert _ok(A.verdict("ar2", A.emu_allreduce2([x.view(T, -1) for x in xs], rank=rank), want))
    for T in A.FUSED_T:
        assert not _rejects_fused(world, None, T=T)


@pytest.mark.parametrize("H", R.NORM_H)
def test_fused_probe_stays_inside_the_measured_rms_limit(H):
    """No new tolerance: over the fused probes the emulation's error is within what row_probes
    measured for rmsnorm_kernel (half the limit the comparison allows)."""
    for world in A.WORLDS:
        f = A.fused(world, H, max(A.WIDE_T, world + 1))
        _, obuf = A.emu_fused(f["xs"], f["res"], f["w"])
        got = obuf[: f["want_out"].numel()].view(f["want_out"].shape)
        assert float(R.excess("rms", got, f["want_out"]).max()) <= R.MEASURED["rms"]
        assert _ok(A.verdict("res", A.emu_fused(f["xs"], f["res"], f["w"], two_shot=True)[0], f["want_res"]))


# (mutant, the family designated to reject it, through the two-shot form)
DESIGNATED = (
    ("drop", "layout", False), ("twice", "layout", False), ("off32", "layout", False), ("block_off", "layout", False),
    ("stale", "layout", False), ("row_off", "layout", True), ("owner_floor", "layout", True), ("no_clamp", "layout", True),
    ("rotate", "order", False), ("bf16_acc", "rounding", False), ("trunc", "rounding", False), ("half_up", "rounding", False),
    ("skip_round", "fused", False), ("skip_round", "fused", True),
)


def test_every_mutant_has_a_designated_family():
    assert {m for m, _, _ in DESIGNATED} == set(A.MUTANTS)
    assert {f for _, f, _ in DESIGNATED} == {"layout", "order", "rounding", "fused"}


@pytest.mark.parametrize("world", A.WORLDS)
@pytest.mark.parametrize("mutant,family,two_shot", DESIGNATED)
def test_mutant_is_rejected(world, mutant, family, two_shot):
    if world < 3 and mutant in A.NEEDS_WORLD_3:
        # two addends: one order, one rounding -- the mutant computes the same bits, nothing to reject
        xs, want, _ = A.rounding(world, MID)
        assert all(not bool(A.mismatch(A.emu_allreduce(xs, mutant, r), want).any()) for r in range(world))
        return
    if family == "fused":
        assert _rejects_fused(world, mutant, two_shot)
    else:
        assert _rejects_plain(family, world, mutant, two_shot)


@pytest.mark.parametrize("world", A.WORLDS)
def test_what_only_one_family_sees(world):
    """Order and rounding faults pass the layout probe (exact in any order, in bf16), a rotated start
    passes everything but the order probe, the skipped rounding everything but the 257 row."""
    for mutant in ("rotate", "bf16_acc", "trunc", "half_up"):
        assert not _rejects_plain("layout", world, mutant)
    assert not _rejects_plain("rounding", world, "rotate") and not _rejects_fused(world, "rotate")
    if world >= 3:
        assert not _rejects_plain("order", world, "bf16_acc") and not _rejects_plain("order", world, "trunc")
    f = A.fused(world, A.FUSED_H, 5)
    rbuf, _ = A.emu_fused(f["xs"], f["res"], f["w"], mutant="skip_round")
    wrong = A.mismatch(rbuf[: 5 * A.FUSED_H], f["want_res"].reshape(-1)).view(5, -1)
    assert bool(wrong[1].all()) and not bool(wrong[[0, 2, 3, 4]].any())
    assert bool((rbuf[: 5 * A.FUSED_H].view(5, -1)[1].double().abs() == 258).all())


@pytest.mark.parametrize("world", A.WORLDS)
def test_fused_probe_rejects_misplaced_reads(world):
    for mutant in ("drop", "twice", "off32", "row_off", "stale"):
        assert _rejects_fused(world, mutant) and _rejects_fused(world, mutant, True), mutant
    for mutant in ("owner_floor", "no_clamp"):
        assert _rejects_fused(world, mutant, True), mutant
        assert not _rejects_fused(world, mutant), "the one-shot form has no owner slices"


# ---------------------------------------------------------------- finding 1, shapes, arms
def _old_vals(n, r, it=0, mod=32):
    return ((torch.arange(n) * (r + 1) + it) % mod).to(BF)


@pytest.mark.parametrize("world", A.WORLDS)
def test_the_old_periodic_data_accepts_misplaced_reads(world):
    """What tests/test_xgmi_ar_gpu.py used before: period 32 in the element index on every rank, so
    a read 32 elements, one block slice or one row (H 1024) away sums to the same integers."""
    n = 8 * 4096 * 3
    xs = [_old_vals(n, r) for r in range(world)]
    want = sum(x.float() for x in xs)
    assert all(torch.equal(x[32:], x[:-32]) for x in xs)
    for mutant in ("off32", "block_off"):
        assert torch.equal(A.emu_allreduce(xs, mutant).float(), want)
    rows = [x.view(-1, 1024) for x in xs]
    assert torch.equal(A.emu_allreduce(rows, "row_off").float().reshape(-1), want)
    for mutant in ("rotate", "bf16_acc", "trunc", "half_up"):
        assert torch.equal(A.emu_allreduce(xs, mutant, world - 1).float(), want)
    # the same faults on the layout probe's data, as that file uses now
    ys, ywant = A.layout(world, n)
    for mutant in ("off32", "block_off"):
        assert bool(A.mismatch(A.emu_allreduce(ys, mutant), ywant).any())
    assert bool(A.mismatch(A.emu_allreduce([y.view(-1, 1024) for y in ys], "row_off").reshape(-1), ywant).any())


def _arm(H):
    """The ROW_DISPATCH arm (MAXV, NW) of csrc/rowcfg.h for a row of H."""
    nw, maxv = R.row_cfg(H)
    if nw < 4:
        return (maxv, nw)
    return (next(m for m in (1, 2, 4, 8) if maxv <= m), 4)


def test_shapes_reach_every_arm_and_edge():
    assert {_arm(H) for H in R.NORM_H} == {(1, 1), (2, 1), (1, 2), (1, 4), (2, 4), (4, 4), (8, 4)}
    assert _arm(8) == (1, 1) and _arm(1032) == _arm(2040) == (1, 4) and _arm(4104) == (4, 4) and _arm(16384) == (8, 4)
    assert [A.plain_blocks(n) for n in A.PLAIN_N] == [(1, 1), (1, 511), (1, 512), (2, 257), (32, 513), (32, 1537)]
    assert A.two_shot_T(2) == (1, 2, 3, 5, 67) and A.two_shot_T(3) == (1, 2, 3, 4, 7, 100)
    assert A.two_shot_T(8) == (1, 7, 8, 9, 17, 265)
    for world in A.WORLDS:
        Ts = A.two_shot_T(world)
        n = lambda T: -(-T // world)  # noqa: E731
        assert n(Ts[-1]) > A.BLOCKS and any(n(T) * (world - 1) >= T for T in Ts), "rows per owner > blocks; an empty owner"
        assert any(0 < T - n(T) * (world - 1) < n(T) for T in Ts), "a short last owner"
    assert max(A.FUSED_T) > 2 * A.BLOCKS and A.BLOCKS in A.FUSED_T
