"""Sampler controls on the device (csrc/sampling.hip lk_sample with 12-wide rows and the bias
operand) against the fp32 reference: logit_bias, presence / frequency penalty counted from the
history ring, the min-p cut, and three concurrent requests through the engine."""
import numpy as np
import pytest
import torch

from llm_kubernetes_minikube_sharp4dev_amd import ops
from llm_kubernetes_minikube_sharp4dev_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = float("inf")


def _prm(B, temp=0.0, top_k=0, top_p=1.0, pen=1.0, last_n=64, reset=0, min_p=0.0, presence=0.0, frequency=0.0,
         width=12, seeds=None):
    """Parameter rows; every argument a scalar or one value per row."""
    prm = np.zeros((B, width), dtype=np.int32)
    f = prm.view(np.float32)
    f[:, 0], f[:, 1], f[:, 2] = temp, top_p, pen
    prm[:, 3], prm[:, 4] = top_k, last_n
    prm[:, 5] = np.arange(B)
    prm[:, 6] = reset
    prm[:, 7] = np.arange(B) if seeds is None else seeds
    if width == 12:
        f[:, 8], f[:, 9], f[:, 10] = min_p, presence, frequency
    return torch.from_numpy(prm)


def _csr(rows: list) -> torch.Tensor:
    """[B+1 offsets | n ids | n f32 bits] of one {id: value} dict (or None) per row."""
    offs, ids, vals = [0], [], []
    for d in rows:
        for t, v in (d or {}).items():
            ids.append(t)
            vals.append(v)
        offs.append(len(ids))
    return torch.from_numpy(np.concatenate([np.asarray(offs, np.int32), np.asarray(ids, np.int32),
                                            np.asarray(vals, np.float32).view(np.int32)]))


# --------------------------------------------------------------------------- penalty arithmetic
W = 256
PEN = [1.3, 1.0, 1.0, 1.7, 1.0, 1.25, 1.1, 1.7]
PRES = [0.0, 0.0, 1.5, 0.3, 0.0, 0.7, -0.25, 0.3]
FREQ = [0.0, 0.75, 0.0, 0.2, 0.0, 0.15, -0.5, 0.2]
LAST_N = [64, 100, -1, 37, 64, -1, 5, 0]     # row 0: legacy-like (every new field zero); row 7: window off
HLEN = [300, 513, 700, 257, 40, 1000, 333, 400]  # all but one longer than the ring


def _case(V):
    """B = 8 greedy rows, one setting each; rings of runs of 1..5 equal tokens (the windows cut
    through a run), logits a shuffle of distinct half-integers."""
    B = 8
    g = torch.Generator().manual_seed(V)
    logits = torch.stack([(torch.randperm(V, generator=g).float() - V // 2) * 0.5 for _ in range(B)])
    hist = torch.zeros(B, W, dtype=torch.int32)
    for r in range(B):
        seq, k = [], 0
        while len(seq) < HLEN[r]:
            seq += [(k * 7 + 3 * r) % V] * (k % 5 + 1)
            k += 1
        for i, t in enumerate(seq[: HLEN[r]]):
            hist[r, i % W] = t
    hist[3, (HLEN[3] - 2) % W] = -1      # entries outside the vocabulary are skipped
    hist[3, (HLEN[3] - 3) % W] = V + 5
    hl = torch.tensor(HLEN, dtype=torch.int32)
    top = [int(logits[r].argmax()) for r in range(B)]
    bias = [None] * B
    bias[4] = {top[4]: -100.0, 1: 7.5, V - 1: 0.25, V: 50.0, -3: 50.0}      # bias only; two ids out of range
    bias[5] = {top[5]: -3.0, int(hist[5, (HLEN[5] - 1) % W]): 2.5}          # a biased token inside the window
    bias[7] = {2: 1000.0}
    logits[6, 9] = -INF                                                      # a masked entry under a bias
    bias[6] = {9: 100.0}
    prm = _prm(B, pen=PEN, presence=PRES, frequency=FREQ, last_n=LAST_N)
    return logits, prm, hist, hl, _csr(bias), bias


def _bound(logits, bias, hist, hl, V):
    """Per element: (c + 2) * 2^-23 * (|rp(l)| + |presence| + c * |frequency|) for the window's
    tokens (fp32, c + 2 dependent operations), 0 everywhere else (untouched or bias only)."""
    B = logits.shape[0]
    bound = torch.zeros_like(logits, dtype=torch.float64)
    for r in range(B):
        if LAST_N[r] == 0:
            continue
        l = logits[r].double().clone()
        for t, v in (bias[r] or {}).items():
            if 0 <= t < V:
                l[t] += v
        n = min(HLEN[r], LAST_N[r] if LAST_N[r] > 0 else W, W)
        toks = [int(hist[r, (HLEN[r] - 1 - j) % W]) for j in range(n)]
        cnt = np.bincount([t for t in toks if 0 <= t < V], minlength=V)
        for t in np.nonzero(cnt)[0]:
            c = int(cnt[t])
            rp = l[t] / PEN[r] if l[t] > 0 else l[t] * PEN[r]
            if torch.isfinite(rp):
                bound[r, t] = (c + 2) * 2.0 ** -23 * (abs(float(rp)) + abs(PRES[r]) + c * abs(FREQ[r]))
    return bound


@pytest.mark.parametrize("V", [1000, 33])
def test_penalty_arithmetic_matches_reference(hip, V):
    logits, prm, hist, hl, csr, bias = _case(V)
    l_ref, h_ref, n_ref = logits.clone(), hist.clone(), hl.clone()
    want = ref.sample(l_ref, prm, h_ref, n_ref, 0, csr)

    def run():
        lg, hd, ld = logits.to(DEV), hist.to(DEV), hl.to(DEV)
        out = ops.sample(lg, prm.to(DEV), hd, ld, 0, bias=csr.to(DEV))
        return out.cpu(), lg.cpu(), hd.cpu(), ld.cpu()

    got, lg, hd, ld = run()
    bound = _bound(logits, bias, hist, hl, V)
    fin = torch.isfinite(l_ref)
    err = (lg.double() - l_ref.double())[fin].abs()
    print("V", V, "tokens", got.tolist(), "max err", float(err.max()), "max err / bound (where bound > 0)",
          float((err / bound[fin].clamp_min(1e-300))[bound[fin] > 0].max()))
    assert torch.equal(got, want.cpu())
    assert torch.equal(lg[~fin], l_ref[~fin]) and lg[6, 9].item() == -INF
    assert (err <= bound[fin]).all()
    assert torch.equal(hd, h_ref) and torch.equal(ld, n_ref)
    # the rows did what their settings say
    assert torch.equal(lg[7], torch.where(torch.arange(V) == 2, logits[7] + 1000.0, logits[7])) and int(got[7]) == 2
    assert (lg[1] != logits[1]).sum() > 0 and (lg[2] != logits[2]).sum() > 0
    changed4 = (lg[4] != logits[4]).nonzero().flatten().tolist()
    assert sorted(changed4) == sorted({t for t in bias[4] if 0 <= t < V})
    # the same launch again on the same inputs: the same bits
    got2, lg2, hd2, ld2 = run()
    assert torch.equal(got2, got) and torch.equal(lg2.view(torch.int32), lg.view(torch.int32)) and torch.equal(hd2, hd)


def test_width_8_equals_width_12_with_zeros(hip):
    torch.manual_seed(5)
    V, B, Wr = 4096, 256, 64
    logits = torch.randn(B, V) * 3
    hist = torch.randint(0, 300, (B, Wr), dtype=torch.int32)
    hl = torch.randint(0, 150, (B,), dtype=torch.int32)
    logits[:, :300] += 4.0
    kw = dict(temp=0.8, top_k=40, top_p=0.9, pen=1.1, last_n=64)

    def run(width, bias=None):
        lg, hd, ld = logits.to(DEV), hist.to(DEV), hl.to(DEV)
        out = ops.sample(lg, _prm(B, width=width, **kw).to(DEV), hd, ld, 99, bias=bias)
        return out.cpu(), lg.cpu().view(torch.int32), hd.cpu(), ld.cpu()

    a = run(8)
    for other in (run(12), run(8, _csr([None] * B).to(DEV)), run(12, _csr([None] * B).to(DEV))):
        assert all(torch.equal(x, y) for x, y in zip(a, other))
    assert len(set(a[0].tolist())) > 20 and (a[1] != logits.view(torch.int32)).any()


# --------------------------------------------------------------------------- min_p
def _expected(row, temp, top_k, top_p, min_p):
    """fp64 probabilities of the reference chain over one logits row."""
    v, idx = torch.sort(row.double(), descending=True, stable=True)
    v, idx = v[:top_k], idx[:top_k]
    e = torch.exp((v - v[0]) / temp)
    incl = torch.cumsum(e, 0)
    keep = ((incl - e) <= top_p * incl[-1]) & (e >= min_p)
    keep[0] = True
    p = torch.zeros_like(row, dtype=torch.float64)
    p[idx[keep]] = e[keep] / e[keep].sum()
    return p


@pytest.mark.parametrize("temp,top_k,top_p,min_p", [(0.8, 40, 0.9, 0.1), (1.0, 0, 1.0, 0.3)])
def test_min_p_distribution(hip, temp, top_k, top_p, min_p):
    V, B = 257, 8192
    g = torch.Generator().manual_seed(2)
    base = torch.randn(V, generator=g) * 2.0
    p = _expected(base, temp, top_k if top_k > 0 else V, top_p, min_p)
    # the thresholds stay clear of equality (the device takes exponents with __expf)
    v = torch.sort(base.double(), descending=True).values
    assert ((torch.exp((v - v[0]) / temp) / min_p - 1).abs() > 1e-3).all()
    logits = base.repeat(B, 1).to(DEV)
    hist = torch.zeros(B, 64, dtype=torch.int32, device=DEV)
    hl = torch.zeros(B, dtype=torch.int32, device=DEV)
    out = ops.sample(logits, _prm(B, temp, top_k, top_p, reset=1, min_p=min_p).to(DEV), hist, hl, seed=321)
    counts = torch.bincount(out.long().cpu(), minlength=V).double()
    # top-p alone keeps more: the min-p cut is what this test sees
    assert int((p > 0).sum()) < int((_expected(base, temp, top_k if top_k > 0 else V, top_p, 0.0) > 0).sum())
    print("support", int((p > 0).sum()), "drawn", int((counts > 0).sum()))
    assert counts[p == 0].sum() == 0, "token outside the top-p / min-p support"
    sigma = torch.sqrt(B * p * (1 - p)) + 1.0
    assert ((counts - B * p).abs() <= 5 * sigma).all()


# --------------------------------------------------------------------------- long ring
def test_frequency_counts_over_a_ring_sized_to_a_long_context(hip):
    """last_n = -1 over a 32,768-entry ring: with zero logits, no repeat penalty and frequency 1 the
    edited logit of a token is minus its count (exact in fp32)."""
    Wl, V, B = 32768, 1000, 2
    rng = np.random.default_rng(0)
    pool = rng.choice(V, 50, replace=False)
    stream = pool[rng.integers(0, 50, 40000)]
    hist = np.zeros((B, Wl), dtype=np.int32)
    hist[0, :20000] = stream[:20000]                # 20,000 entries, not wrapped
    for i, t in enumerate(stream):                   # 40,000 entries: the ring holds the last 32,768
        hist[1, i % Wl] = t
    hl = torch.tensor([20000, 40000], dtype=torch.int32)
    logits = torch.zeros(B, V, device=DEV)
    ops.sample(logits, _prm(B, last_n=-1, frequency=1.0).to(DEV), torch.from_numpy(hist).to(DEV), hl.to(DEV))
    got = (-logits).cpu().numpy()
    assert np.array_equal(got[0], np.bincount(stream[:20000], minlength=V).astype(np.float32))
    assert np.array_equal(got[1], np.bincount(stream[40000 - Wl:], minlength=V).astype(np.float32))
    assert got[0].sum() == 20000 and got[1].sum() == Wl


# --------------------------------------------------------------------------- grammar mask
def test_grammar_masked_rows_with_bias_and_penalties(hip):
    torch.manual_seed(6)
    V, B = 128256, 32
    logits = torch.full((B, V), -INF, device=DEV)
    allowed = torch.stack([torch.randperm(V)[:3] for _ in range(B)]).to(DEV)
    for j in range(3):
        logits[torch.arange(B, device=DEV), allowed[:, j]] = torch.randn(B, device=DEV)
    hist = torch.randint(0, V, (B, 64), dtype=torch.int32, device=DEV)
    hl = torch.full((B,), 64, dtype=torch.int32, device=DEV)
    hist[:, 0] = hist[:, 1] = allowed[:, 0].int()  # an allowed id twice in the window
    al = allowed.cpu().tolist()
    # +100 on a masked id (it stays masked), -100 on the first allowed one
    bias = _csr([{next(x for x in range(4) if x not in a): 100.0, a[0]: -100.0} for a in al])
    kw = dict(pen=1.1, presence=0.5, frequency=0.5, last_n=64)
    out = ops.sample(logits.clone(), _prm(B, 0.8, 40, 0.9, min_p=0.05, **kw).to(DEV), hist, hl, seed=11,
                     bias=bias.to(DEV))
    assert (out[:, None].long() == allowed[:, 1:]).any(1).all()  # e^(-100 / 0.8) is below min_p: never the first
    g = ops.sample(logits.clone(), _prm(B, 0.0, 40, **kw).to(DEV), hist, hl, bias=bias.to(DEV))
    assert (g[:, None].long() == allowed[:, 1:]).any(1).all()


def test_binding_rejects_bad_operands(hip):
    lg = torch.zeros(2, 64, device=DEV)
    hist, hl = torch.zeros(2, 8, dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):
        ops.sample(lg, torch.zeros(2, 10, dtype=torch.int32, device=DEV), hist, hl)
    with pytest.raises(RuntimeError):
        ops.sample(lg, _prm(2).to(DEV), hist, hl, bias=_csr([None, None]))               # on the host
    with pytest.raises(RuntimeError):
        ops.sample(lg, _prm(2).to(DEV), hist, hl, bias=torch.zeros(2, dtype=torch.int32, device=DEV))  # < B + 1


# --------------------------------------------------------------------------- engine
@pytest.mark.parametrize("graphs", [False, True])
def test_engine_three_concurrent_requests(monkeypatch, graphs):
    from test_engine_gpu import PROMPTS, _engine, _gpu_llama

    from llm_kubernetes_minikube_sharp4dev_amd.engine.sampling import SamplingParams

    monkeypatch.setenv("LK_DECODE_TUNE", "0")
    m = _gpu_llama()[1]
    T = 77
    mk = [lambda: SamplingParams.greedy(24, frequency_penalty=1e4, repeat_last_n=-1, ignore_eos=True),
          lambda: SamplingParams.greedy(24, logit_bias={T: 100.0}),
          lambda: SamplingParams.greedy(24)]

    def run(which):
        eng = _engine(m, use_graphs=graphs)
        if graphs:
            eng.runner.capture_all(max_batch=8)
        seqs = [eng.add_request(PROMPTS[i], mk[i]()) for i in which]
        while eng.has_work():
            eng.step_pipelined()
        eng.flush()
        return [s.output_ids for s in seqs]

    a, b, c = run([0, 1, 2])
    print("frequency", a, "bias", b, "plain", c)
    assert len(a) == 24 and len(set(a)) == 24
    assert b == [T] * 24
    assert c == run([2])[0]
