"""MMR selection without a GPU: the integer model of tests/mmr_probes.py against ``ops.mmr_select`` on CPU
tensors (the fp32 reference) bit for bit, the patterns the probes have to contain, and the refusals."""
import numpy as np
import pytest
import torch

import mmr_probes as P
from llm_kubernetes_minikube_sharp4dev_amd import ops


@pytest.mark.parametrize("D", P.SWEEP_D)
def test_reference_equals_the_model_bit_for_bit(D):
    for d, C, K, nq, lam4 in P.sweep():
        if d != D:
            continue
        case = P.make_case(D, C, K, nq, lam4)
        corpus, cn, cid, rel, lam = P.tensors(case)
        for fn in (ops.mmr_select, ops.reference.mmr_select):
            P.check_exact(fn(corpus, cn, cid, rel, lam, K), case, (D, C, K, nq, lam4))


@pytest.mark.parametrize("lam4", P.LAMS4)
def test_every_lambda_on_the_full_width(lam4):
    case = P.make_case(128, 64, 64, 3, lam4)
    corpus, cn, cid, rel, lam = P.tensors(case)
    P.check_exact(ops.mmr_select(corpus, cn, cid, rel, lam, 64), case, lam4)


def test_probe_patterns_are_present():
    for D in P.SWEEP_D:
        X = P.corpus(D).astype(np.int64)
        G = X @ X.T
        assert np.all(np.diag(G) == 16)
        assert all(G[0, i] == 16 for i in P.COPIES)            # exact copies: sim 1
        assert all(G[0, i] == -16 for i in P.OPPOSITE)         # opposite rows: sim -1
        assert G[P.ORTHO[0], P.ORTHO[1]] == 0                  # an orthogonal pair: sim 0
        assert len(np.unique(G)) > 8 or D == 16                # and many values in between
    case = P.make_case(128, 64, 10, 3, 2)
    ids, r16, nan = case["ids"], case["r16"], case["nan"]
    pos, oid, rel, mmr, sim = P.expected(case)
    row = ids[0]
    assert 0 in row and P.N - 1 in row                         # ids 0 and N - 1
    assert row[35] == -1 and row[36] == P.N and row[37] == 2 ** 31 - 1 and row[63] == -1 and nan[0, 21]
    assert row[5] == row[4]                                    # a duplicated id
    assert not {21, 35, 36, 37, 63} & set(pos[0].tolist())     # the absent ones are never picked
    # lam = 1/2.  Positions 0, 1, 7 (first 32) and 31, 32 (across the boundary) are copies of one row
    # with rel 12/16: equal mmr in every round, so they come out in position order, and from the second
    # on each reports max_sim = 1
    full = P.model(case["X"], ids, r16, nan, 2, 64)
    assert [p for p in full[0][0].tolist() if p in (0, 1, 7, 31, 32)] == [0, 1, 7, 31, 32]
    whole = dict(zip(full[0][0].tolist(), full[4][0].tolist()))
    assert all(whole[p] == 1.0 for p in (1, 7, 31, 32))
    mm = dict(zip(full[0][0].tolist(), full[3][0].tolist()))
    assert mm[1] == mm[7] == mm[31] == mm[32] == np.float32((2 * 12 - 2 * 16) / 64)
    npres = int(((ids[0] >= 0) & (ids[0] < P.N) & ~nan[0]).sum())
    assert full[0][0].tolist().count(-1) == 64 - npres         # pads once the present ones ran out
    assert (pos[1] >= 0).sum() == 9 and pos[1, 9] == -1 and np.isinf(mmr[1, 9])   # fewer present than K
    assert np.all(pos[2] == -1) and np.all(oid[2] == -1) and np.all(np.isinf(rel[2]))  # none present
    # a negative similarity stays negative in max_sim: only the opposite row selected first
    X = case["X"]
    two = P.model(X, np.array([[0, P.N - 1]]), np.array([[16, 16]]), np.zeros((1, 2), bool), 2, 2)
    assert two[0].tolist() == [[0, 1]] and two[4].tolist() == [[0.0, -1.0]] and two[3].tolist() == [[0.5, 1.0]]
    # and the signed zero of the model: lam = 0, rel < 0, first round
    z = P.model(X, np.array([[7]]), np.array([[-8]]), np.zeros((1, 1), bool), 0, 1)
    assert np.signbit(z[3][0, 0]) and z[3][0, 0] == 0


def test_refusals_and_the_call_after_them():
    case = P.make_case(48, 33, 6, 3, 1)
    corpus, cn, cid, rel, lam = P.tensors(case)
    bad = [
        (r"C \(the width of cand_id\) must be in \[1, 64\]", (corpus, cn, cid.repeat(1, 2), rel.repeat(1, 2), lam, 6)),
        (r"C \(the width of cand_id\)", (corpus, cn, cid[:, :0], rel[:, :0], lam, 1)),
        (r"K must be", (corpus, cn, cid, rel, lam, 0)),
        (r"K must be", (corpus, cn, cid, rel, lam, 34)),
        (r"K must be", (corpus, cn, cid, rel, lam, 2.0)),
        (r"D must be a multiple of 16", (corpus[:, :40].contiguous(), cn, cid, rel, lam, 6)),
        (r"D must be a multiple of 16", (corpus[:, :0].contiguous(), cn, cid, rel, lam, 6)),
        (r"D must be a multiple of 16", (corpus.repeat(1, 22), cn, cid, rel, lam, 6)),      # 1056 > 1024
        (r"lam must be a finite number in \[0, 1\]", (corpus, cn, cid, rel, 1.5, 6)),
        (r"lam must be", (corpus, cn, cid, rel, -0.25, 6)),
        (r"lam must be", (corpus, cn, cid, rel, float("nan"), 6)),
        (r"lam must be", (corpus, cn, cid, rel, float("inf"), 6)),
        (r"lam must be", (corpus, cn, cid, rel, "0.5", 6)),
        (r"same shape", (corpus, cn, cid, rel[:, :-1], lam, 6)),
        (r"same shape", (corpus, cn, cid[0], rel[0], lam, 6)),
        (r"corpus must be bfloat16", (corpus.float(), cn, cid, rel, lam, 6)),
        (r"cnorm must be float32 \[N\]", (corpus, cn.double(), cid, rel, lam, 6)),
        (r"cnorm must be float32 \[N\]", (corpus, cn[:-1], cid, rel, lam, 6)),
        (r"cand_id must be int32", (corpus, cn, cid.long(), rel, lam, 6)),
        (r"rel must be float32", (corpus, cn, cid, rel.double(), lam, 6)),
    ]
    for match, args in bad:
        for fn in (ops.mmr_select, ops.reference.mmr_select):
            with pytest.raises(ValueError, match=match):
                fn(*args)
            P.check_exact(fn(corpus, cn, cid, rel, lam, 6), case, match)
    # N >= 2^31 is refused by the shape alone (no such tensor is made here)
    with pytest.raises(ValueError, match=r"N must be below 2\^31"):
        ops.reference.mmr_check(torch.zeros(1, 16, dtype=torch.bfloat16).expand(2 ** 31, 16),
                                torch.zeros(1).expand(2 ** 31), cid, rel, lam, 6)
    # no queries / no corpus rows: empty outputs, every candidate absent
    out = ops.mmr_select(corpus, cn, cid[:0], rel[:0], lam, 6)
    assert [tuple(o.shape) for o in out] == [(0, 6)] * 5
    out = ops.mmr_select(corpus[:0], cn[:0], cid, rel, lam, 6)
    assert torch.all(out[0] == -1) and torch.all(out[1] == -1) and all(torch.all(torch.isinf(o)) for o in out[2:])
