"""The attention probes of tests/attn_probes.py can fail: a CPU emulation of the kernels' flash
arithmetic passes them at every shape the GPU tests use, and every mutant -- a wrong answer a
broken kernel would give -- is rejected by at least one of the probes U / N / W on every row it
alters.  Also: the q_past / partials arguments of ops.reference.flash_prefill against the probes'
float64 answers."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_probes as P  # noqa: E402

from llm_kubernetes_minikube_sharp4dev_amd import ops  # noqa: E402
from llm_kubernetes_minikube_sharp4dev_amd.ops import reference as ref  # noqa: E402


def test_probes_pass_under_emulated_flash_arithmetic():
    """Every probe at every shape of the GPU tests: the emulated kernel's bf16 answer is within the
    probe's tolerance of the float64 answer, expected zeros are exact zeros, and the floor of the
    comparison is below 1/16 of the smallest non-zero expected element."""
    count = 0
    for label, probe, split, k0, defers in P.shapes():
        for s in range(len(probe.k)):
            for defer in defers:
                got, _, want = P.emulate_seq(probe, s, split, k0, defer)
                P.check(probe.kind, got, want, f"{label} sequence {s} defer {defer}")
            nz = want[want != 0].abs()
            assert nz.numel() == 0 or P.FLOOR < float(nz.min()) / 16
            count += 1
    assert count > 500


def test_needle_is_one_key_to_a_bf16_ulp():
    """The needle probe's float64 answer is the V row of the key asked for: every other key
    weighs less than e^-39 of it."""
    probe = P.build("N", P.decode_geom([1, 17, 129, 4097]), 2, 1, 64, split=128)
    for r in range(probe.B):
        s = probe.seq[r]
        code = probe.q[r][0].double()  # [Hq, D]
        for h in range(probe.Hq):
            scores = probe.k[s][:, h // probe.G].double() @ code[h]
            j = int(scores.argmax())
            rest = torch.cat([scores[:j], scores[j + 1:]])
            assert rest.numel() == 0 or float(scores[j] - rest.max()) * probe.scale > 39.0
            v = probe.v[s][j, h // probe.G].double()
            assert float((probe.want(r)[0, h] - v).abs().max()) < 1e-12


def test_weighted_and_staircase_tolerances_are_twice_the_emulation_error():
    worst = P.measure_rtol()
    print()
    for kind, const in (("W", P.RTOL_W), ("S", P.RTOL_S)):
        e, where = worst[kind]
        print(f"probe {kind}: emulation error {100 * e:.3f} % at {where}; rtol {100 * const:.3f} %")
        assert 2 * e <= const <= 2 * e * 1.01


def _mutant_configs():
    """Every decode, cascade and prefill shape at G 4, D 128; a cascade and the prefill batch at G 1,
    D 64, where a kv head has a single query head (a prefill row then asks for two needles only)."""
    for G, D, splits, prefixes in ((4, 128, (128, 2048), P.CASCADE_PREFIX_BLOCKS), (1, 64, (128,), (3,))):
        for split in splits:
            if G == 4:
                yield (f"decode G{G} D{D} split{split}", P.decode_geom(P.DECODE_CTX), G, D, True,
                       dict(BS=16, split=split, k_start=0))
            for S in prefixes:
                geom = P.decode_geom([S * 16 + t for t in P.CASCADE_TAILS])
                yield (f"cascade G{G} D{D} split{split} prefix{S}", geom, G, D, True,
                       dict(BS=16, split=split, k_start=S * 16, cascade=True))
        # prefill: the tile of 64 keys takes the place of the split
        yield f"prefill G{G} D{D}", P.prefill_geom(P.PREFILL_QP), G, D, True, dict(BS=16, split=64, k_start=0)
    yield "decode G4 D128 BS128", P.decode_geom(P.DECODE_CTX), 4, 128, True, dict(BS=128, split=2048, k_start=0)


def test_every_mutant_is_rejected_on_every_row_it_alters():
    """Per mutant, the smallest |wrong - want| / tolerance over the rows it alters, each row judged
    by the best of U, N and W (a probe may let a mutant through on a row where another rejects
    it): above 1 everywhere.  A row counts as altered where the mutant changes the keys it sees."""
    table = {name: (float("inf"), "not applicable") for name in P.MUTANTS}
    for label, geom, G, D, causal, cfg in _mutant_configs():
        probes = {kind: P.build(kind, geom, 2, G, D, causal, split=cfg["split"], BS=cfg["BS"],
                                k_start=cfg["k_start"]) for kind in "UNW"}
        for name in P.MUTANTS:
            for s, (n, ql, _) in enumerate(geom):
                best = torch.zeros(ql)
                altered = torch.zeros(ql, dtype=torch.bool)
                by = ["-"] * ql
                for kind, probe in probes.items():
                    for r in probe.rows_of_seq(s):
                        out = P.mutate(name, probe, r, cfg)
                        if out is None:
                            continue
                        wrong, alt = out
                        altered |= alt
                        x = P.excess(kind, wrong, probe.want(r)).flatten(1).amax(dim=1)
                        for i in torch.nonzero(x > best).flatten().tolist():
                            by[i] = kind
                        best = torch.maximum(best, x)
                if name.startswith("swap"):
                    # cache blocks 0 and 8 of U and W hold the same V rows (the pattern has period D), and a
                    # needle query weighs one key: a swap alters the rows whose answer it changes in some probe
                    altered &= best > 1e-6
                for i in torch.nonzero(altered).flatten().tolist():
                    assert float(best[i]) > 1, (f"mutant '{name}' passes every probe at {label}, {n} keys, query row {i}: "
                                                f"{float(best[i]):.3g} x tolerance")
                    if float(best[i]) < table[name][0]:
                        table[name] = (float(best[i]), f"{label}, {n} keys, query row {i}, by {by[i]}")
    print()
    print(f"{'mutant':34s} smallest error / tolerance over the rows it alters")
    for name, (x, where) in table.items():
        print(f"{name:34s} {x:10.3g}  {where}")
        assert x != float("inf"), f"mutant '{name}' never applied"


def _shard_problem(kind):
    probe = P.build(kind, P.SHARD_GEOM, 2, 4, 128)
    kc, vc, bt, ctx = P.to_paged(probe, 16)
    q = torch.cat(probe.q).reshape(-1, probe.Hq * probe.D)
    ql = [probe.qlen(r) for r in range(probe.B)]
    cu = torch.tensor([0] + torch.tensor(ql).cumsum(0).tolist(), dtype=torch.int32)
    return probe, q, kc, vc, bt, ctx, cu, torch.tensor(probe.past, dtype=torch.int32)


@pytest.mark.parametrize("kind", ["U", "W"])
def test_reference_q_past_and_partials(kind):
    """ops.reference.flash_prefill with q_past: the bf16 output and the (o, m, l) partials against
    the probe's float64 answer; rows that see no key have o = 0, m = -inf, l = 0.  The CPU path of
    ops.flash_prefill fills ``part`` with the same."""
    probe, q, kc, vc, bt, ctx, cu, qp = _shard_problem(kind)
    want = probe.want_all()
    lse2 = torch.cat([probe.lse2(r) for r in range(probe.B)])
    y = ref.flash_prefill(q, kc, vc, bt, cu, ctx, probe.Hq, 2, 128, probe.scale, True, q_past=qp)
    P.check("U", y.reshape(want.shape), want, "reference output")  # one bf16 rounding of the exact answer
    o, m, l = ref.flash_prefill(q, kc, vc, bt, cu, ctx, probe.Hq, 2, 128, probe.scale, True, q_past=qp,
                                partials=True)
    blind = torch.isinf(lse2)
    assert bool(blind.any()) and bool((~blind).any())
    assert bool((l[blind] == 0).all()) and bool((o[blind] == 0).all()) and bool((m[blind] == float("-inf")).all())
    torch.testing.assert_close((o / l[..., None])[~blind].double(), want[~blind], rtol=1e-5, atol=0)
    torch.testing.assert_close((m + torch.log2(l))[~blind].double(), lse2[~blind], rtol=1e-5, atol=1e-5)
    po = torch.empty(q.shape[0], probe.Hq, 128)
    pml = torch.empty(q.shape[0], probe.Hq, 2)
    ops.flash_prefill(q, kc, vc, cu, probe.Hq, 2, 128, probe.scale, True, block_tables=bt, ctx_lens=ctx,
                      part=(po, pml), q_past=qp)
    assert torch.equal(po, o) and torch.equal(pml[..., 0], m) and torch.equal(pml[..., 1], l)
    y2 = ops.flash_prefill(q, kc, vc, cu, probe.Hq, 2, 128, probe.scale, True, block_tables=bt, ctx_lens=ctx, q_past=qp)
    assert torch.equal(y2, y)


def test_reference_default_past_is_unchanged():
    """Without q_past the reference attends as before (past = ctx_len - q_len)."""
    probe = P.build("W", P.prefill_geom(P.PREFILL_QP), 2, 2, 64)
    kc, vc, bt, ctx = P.to_paged(probe, 16)
    q = torch.cat(probe.q).reshape(-1, probe.Hq * 64)
    cu = torch.tensor([0] + torch.tensor([probe.qlen(r) for r in range(probe.B)]).cumsum(0).tolist(), dtype=torch.int32)
    y = ref.flash_prefill(q, kc, vc, bt, cu, ctx, probe.Hq, 2, 64, probe.scale, True)
    y2 = ref.flash_prefill(q, kc, vc, bt, cu, ctx, probe.Hq, 2, 64, probe.scale, True,
                           q_past=torch.tensor(probe.past, dtype=torch.int32))
    want = probe.want_all()
    P.check("U", y.reshape(want.shape), want, "default past")
    P.check("U", y2.reshape(want.shape), want, "explicit past")
