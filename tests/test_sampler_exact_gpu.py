"""The token selectors of csrc/sampling.hip against the CPU model of tests/sampler_probes.py, which
knows the token every (engine seed, request seed, position) must produce: sample_topkp_kernel on exact
probes (plateaus: integer prefixes, no tolerance), on the radix fallback and on random rows with a
margin, select_kernel's Gumbel path for f32 / bf16 / grammar rows, the draws that were u == 1, and the
order of -0.0 and +0.0.  tests/test_sampler_probes_cpu.py shows which kernel mistakes these inputs
catch and that the random rows are pinned often enough."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_probes as P  # noqa: E402

from llm_kubernetes_minikube_sharp4dev_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """A failed comparison is a result; a device error is not: nothing more runs on the device after one."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, the remaining tests are not run: {e}", returncode=3)


def _run(case):
    """ops.sample on the case -> (tokens, logits after the call, ring, ring lengths) as numpy."""
    logits = torch.from_numpy(case.logits).to(DEV)
    hist = torch.from_numpy(case.hist.copy()).to(DEV)
    hl = torch.from_numpy(case.hl.copy()).to(DEV)
    out = ops.sample(logits, torch.from_numpy(case.prm).to(DEV), hist, hl, seed=case.seed)
    return out.cpu().numpy(), logits.cpu().numpy(), hist.cpu().numpy(), hl.cpu().numpy()


def _check(case, cap=None):
    """Every token inside its admissible set (one token for an exact case), the ring appended at
    position % W and nowhere else, the lengths advanced.  Returns the unpinned share."""
    got, _, hist, hl = _run(case)
    want = case.expected()
    bad = [(r, int(got[r]), sorted(want[r])[:4]) for r in range(len(got)) if int(got[r]) not in want[r]]
    unpinned = sum(len(s) > 1 for s in want) / len(want)
    print(f"{case.name}: {len(bad)} of {len(got)} rows outside their admissible set, unpinned {unpinned:.4f}")
    assert not bad, f"{case.name}: (row, token, admissible) {bad[:8]}"
    if case.exact:
        assert unpinned == 0
    else:  # how much of the tolerance the kernel used: the eps its least certain row needed
        print(f"{case.name}: largest eps a row needed {case.needed_eps(got) / P.EPS:.4f} of EPS = {P.EPS:.3e}")
    if cap is not None:
        assert unpinned <= cap, (case.name, unpinned)
    ring, lens = case.hist.copy(), case.hl.copy()
    for r in range(len(got)):
        slot, pos = int(case.prm[r, 5]), case.position(r)
        ring[slot, pos % case.W], lens[slot] = got[r], pos + 1
    assert np.array_equal(hist, ring) and np.array_equal(hl, lens), case.name
    return got


# ================================================================ sample_topkp_kernel, exact probes
@pytest.mark.parametrize("K", P.PLATEAU_K)
def test_plateau_kept_count_and_pick(hip, K):
    """top_k = K over 1300 ties, every (temperature, top_p), 8- and 12-wide rows: the token is
    order[floor(u * kept)] with kept = floor(top_p * K) + 1 clamped to K and u the exact float32 draw
    (rows with an integer u * 1024 and with the draw that was u == 1 among them: the latter picks the
    last kept candidate)."""
    for width in (8, 12):
        case = P.plateau_case(K, width)
        got = _check(case)
        od = P.order(case.logits[0], K)
        for r in range(3):  # seed 123's rows of _special_seeds: top_p = 1, the last is the u == 1 tuple
            assert P.parse(case.prm[r])["top_p"] == 1.0
        assert got[2] == od[K - 1]


@pytest.mark.parametrize("width", [8, 12])
def test_underflow_level_is_never_picked(hip, width):
    case = P.underflow_case(width)
    got = _check(case)
    assert (case.logits[0][got] == 3.0).all()


def test_min_p_boundary(hip):
    case = P.min_p_case()
    got = _check(case)
    assert (got[1::2] == 1).all() and len(set(got[0::2].tolist())) > 8


@pytest.mark.parametrize("V", P.SIZES_V)
def test_sizes(hip, V):
    _check(P.sizes_case(V))


def test_placement(hip):
    one, many = P.placement_cases()
    a, b = _check(one), _check(many)
    assert a[0] == b[37]


def test_position(hip):
    case = P.position_case()
    got = _check(case)
    assert got[-1] == got[0]  # reset draws at position 0
    assert len(set(got[:-1].tolist())) == len(P.POS_HL)


def test_zero_order(hip):
    """-0.0 at id 0 and +0.0 at id 5 tie: id 0 is the greedy token and candidate 0 of the sampled rows,
    and token_logprobs lists them in id order."""
    case = P.zeros_case()
    got = _check(case)
    assert (got[:8] == 0).all() and set(got[8:].tolist()) == {0, 5}
    for dt in (torch.float32, torch.bfloat16):
        lg = torch.zeros(2, 16, dtype=dt)
        lg[:, :8] = torch.from_numpy(case.logits[:2]).to(dt)
        lg[:, 8:] = -7.0
        for n in (1, 2):  # (n = 1: the bound of the gather is +0.0 itself)
            _, _, top_id = ops.token_logprobs(lg.to(DEV), torch.zeros(2, dtype=torch.int32, device=DEV),
                                              torch.arange(2, dtype=torch.int32, device=DEV), n)
            assert top_id.cpu().tolist() == [[0, 5][:n]] * 2, (dt, n)


# ================================================================ sample_topkp_kernel, radix fallback
@pytest.mark.parametrize("name", list(P.radix_rows()))
def test_radix_fallback(hip, name):
    case = P.radix_case(name)
    assert P.needs_radix(case.logits[0], P.parse(case.prm[0])["top_k"])
    _check(case, cap=0.10)


# ================================================================ sample_topkp_kernel, random rows
@pytest.mark.parametrize("i", range(len(P.RANDOM_SPREADS) * len(P.RANDOM_V) * len(P.RANDOM_PARAMS)))
def test_random_rows_with_margin(hip, i):
    case = P.random_case(i)
    _check(case, cap=P.unpinned_cap(case.prm[0], case.logits.shape[1]))


def test_random_rows_ring_and_repeat_penalty(hip):
    case = P.penalty_case()
    _, logits, _, _ = _run(case)
    assert np.array_equal(logits, np.stack([case.edited(r) for r in range(len(logits))]))
    assert not np.array_equal(logits, case.logits)
    _check(case, cap=0.02)


# ================================================================ select_kernel, temperatures on
def _select_all(hip, l, temps, seed, step, plan=None):
    """f32 and bf16, each on a padded-stride view whose padding holds a larger value than any logit,
    and (with a plan) select_allowed in both types."""
    B, V = l.shape
    S = (V + 24 + 7) // 8 * 8  # rows stay 32-byte aligned
    f = torch.full((B, S), 99.0, dtype=torch.float32, device=DEV)[:, :V]
    f.copy_(torch.from_numpy(l))
    bf = torch.full((B, S), 99.0, dtype=torch.bfloat16, device=DEV)[:, :V]
    bf.copy_(f)
    t = torch.from_numpy(temps).to(DEV)
    if plan is None:
        return [ops.select_tokens(f, t, seed=seed, step=step), ops.select_tokens(bf, t, seed=seed, step=step)]
    return [hip.select_allowed(f, plan, t, seed, step), hip.select_allowed(bf, plan, t, seed, step)]


@pytest.mark.parametrize("V", P.GUMBEL_V)
def test_gumbel_select(hip, V):
    """Every (seed, step): the token is the model's id where the row is pinned and inside the
    admissible set elsewhere; greedy rows (T = 0) and sampled ones mixed in a batch."""
    l, temps = P.gumbel_logits(V), P.gumbel_temps()
    plan_np, allowed = P.allowed_plan(P.GUMBEL_B, V)
    plan = torch.from_numpy(plan_np).to(DEV)
    rows = unpinned = 0
    gap = 0.0
    for seed in P.GUMBEL_SEEDS:
        for step in P.GUMBEL_STEPS:
            full = [P.gumbel(l[r], temps[r], seed, r, step) for r in range(P.GUMBEL_B)]
            part = [P.gumbel(l[r], temps[r], seed, r, step, allowed[r]) for r in range(P.GUMBEL_B)]
            for want, outs in ((full, _select_all(hip, l, temps, seed, step)), (part, _select_all(hip, l, temps, seed, step, plan))):
                for out in outs:
                    got = out.cpu().tolist()
                    bad = [(r, got[r], sorted(want[r])) for r in range(P.GUMBEL_B) if got[r] not in want[r]]
                    assert not bad, (V, hex(seed), step, bad[:6])
                    ids = full is want and [None] * P.GUMBEL_B or allowed
                    gap = max(gap, max(P.gumbel_gap(l[r], temps[r], seed, r, step, got[r], ids[r]) for r in range(P.GUMBEL_B)))
                rows += len(want)
                unpinned += sum(len(s) > 1 for s in want)
    print(f"gumbel V{V}: unpinned {unpinned} of {rows}, largest gap of a chosen score below the best {gap:.3e} "
          f"(admissible up to 2 * EPS_G = {2 * P.EPS_G:.3e})")
    assert unpinned <= 0.01 * rows


@pytest.mark.parametrize("seed,row,step,tok", P.U1_GUMBEL)
def test_gumbel_u_equal_one_does_not_win(hip, seed, row, step, tok):
    """The draw whose u rounded to 1 (Gumbel noise +inf) sits on a logit of -50 beside zeros: it must
    lose, and the row's token is the model's."""
    B, V = row + 1, 2048
    l = np.zeros((B, V), np.float32)
    l[row, tok] = -50.0
    assert (P.gumbel_hash(seed, row, step, tok)[0] >> 8) == 0xFFFFFF
    temps = np.ones(B, np.float32)
    plan = np.concatenate([np.ones(B, np.int32), np.arange(B + 1, dtype=np.int32) * 4, np.tile([3, tok, 77, 2000], B).astype(np.int32)])
    for want_ids, outs in ((None, _select_all(hip, l, temps, seed, step)),
                           ([3, tok, 77, 2000], _select_all(hip, l, temps, seed, step, torch.from_numpy(plan).to(DEV)))):
        want = P.gumbel(l[row], 1.0, seed, row, step, want_ids)
        for out in outs:
            got = int(out[row])
            assert got != tok and got in want, (got, want)
