"""Shared inputs of the cross-encoder score-head tests (CPU reference and lk_rerank_head).

Exact probes.  Entries of x are in {0, +-2, +-4}, of pool_w in {0, +-16, +-32}, of pool_b in
{0, +-32}: every a_j = sum_k w_jk x_k + b_j is a multiple of 32 and exact in fp32 in any
summation order (|a_j| <= 1024*128 + 32 < 2^24).  tanh(32) differs from 1 by 3e-28, so a
correctly rounded tanhf gives exactly 0 or +-1.  cls_w holds integers |c| <= 8 and cls_b is an
integer, so the logit is an exact integer, computed here with numpy int64.  Every value is exactly
representable in bf16.  Every non-CLS row of ``hidden`` is NaN (reading a wrong row poisons the
result) and ``hidden`` is a view with row stride H + 8.
"""
import numpy as np
import torch

LENS = (3, 1, 0, 2, 5, 1, 4)  # cycled: a length-1 and an empty sequence among the first three


def probe_lens(B):
    return [3] if B == 1 else [LENS[i % len(LENS)] for i in range(B)]


def _hidden(xs, lens, H, dtype):
    """[T, H] view (row stride H + 8) of a NaN buffer whose CLS rows are ``xs`` (one per non-empty
    sequence; an empty sequence owns no row), and cu [B+1]."""
    T = int(sum(lens))
    buf = torch.full((max(T, 1), H + 8), float("nan"), dtype=dtype)
    cu = np.zeros(len(lens) + 1, dtype=np.int64)
    cu[1:] = np.cumsum(lens)
    for b, n in enumerate(lens):
        if n > 0:
            buf[int(cu[b]), :H] = torch.from_numpy(xs[b].astype(np.float32)).to(dtype)
    return buf[:T, :H], torch.from_numpy(cu.astype(np.int32))


def exact_probe(H, B, pattern, seed=0, dtype=torch.bfloat16):
    """-> dict(hidden, cu, pool_w, pool_b, cls_w, cls_b, expected int64 [B]); ``pattern``:
    "dense" (random over the value sets) or "onehot" (pool_w row j has a single nonzero at column
    (7j+3) % H: pins each (row, column, bias, classifier) pairing)."""
    rng = np.random.default_rng(seed * 1000 + H + B)
    lens = probe_lens(B)
    x = rng.choice(np.array([0, 2, -2, 4, -4]), size=(B, H))
    if pattern == "dense":
        W = rng.choice(np.array([0, 16, -16, 32, -32]), size=(H, H))
    elif pattern == "onehot":
        W = np.zeros((H, H), dtype=np.int64)
        j = np.arange(H)
        W[j, (7 * j + 3) % H] = rng.choice(np.array([16, -16, 32, -32]), size=H)
        x = rng.choice(np.array([2, -2, 4, -4, 0]), size=(B, H), p=[0.225, 0.225, 0.225, 0.225, 0.1])
    else:
        raise ValueError(pattern)
    pb = rng.choice(np.array([0, 32, -32]), size=H)
    c = rng.integers(-8, 9, size=H)
    cb = int(rng.integers(-5, 6))
    for b, n in enumerate(lens):
        if n == 0:
            x[b] = 0  # an empty sequence pools the zero vector
    a = x.astype(np.int64) @ W.astype(np.int64).T + pb[None, :]
    assert np.all(a % 32 == 0) and np.abs(a).max() < 2 ** 24
    expected = (np.sign(a) * c[None, :]).sum(1) + cb
    hidden, cu = _hidden(x, lens, H, dtype)
    t = lambda v: torch.from_numpy(np.asarray(v, dtype=np.float32)).to(dtype)  # noqa: E731
    return dict(hidden=hidden, cu=cu, pool_w=t(W), pool_b=t(pb), cls_w=t(c).reshape(1, H), cls_b=t([cb]),
                expected=expected.astype(np.int64))


def zero_logit_probe(H, dtype=torch.bfloat16, seed=3):
    """Two sequences whose logit is exactly 0 with nonzero tanh terms: pool_w rows j and j + H/2
    are equal (so are pool_b's entries) and cls_w[j + H/2] = -cls_w[j]; cls_b = 0."""
    rng = np.random.default_rng(seed + H)
    h2 = H // 2
    Wh = rng.choice(np.array([0, 16, -16, 32, -32]), size=(h2, H))
    W = np.concatenate([Wh, Wh])
    pbh = rng.choice(np.array([0, 32, -32]), size=h2)
    pb = np.concatenate([pbh, pbh])
    ch = rng.integers(1, 9, size=h2)
    c = np.concatenate([ch, -ch])
    x = rng.choice(np.array([0, 2, -2, 4, -4]), size=(2, H))
    a = x @ W.T + pb[None, :]
    assert np.count_nonzero(a) > 0 and np.all((np.sign(a) * c[None, :]).sum(1) == 0)
    hidden, cu = _hidden(x, [2, 3], H, dtype)
    t = lambda v: torch.from_numpy(np.asarray(v, dtype=np.float32)).to(dtype)  # noqa: E731
    return dict(hidden=hidden, cu=cu, pool_w=t(W), pool_b=t(pb), cls_w=t(c).reshape(1, H), cls_b=t([0]))


def probe_args(p, device=None):
    """The op's positional tensor arguments, on ``device`` (the hidden view keeps its H + 8 stride:
    the whole buffer moves, then it is sliced again)."""
    h = p["hidden"]
    if device is not None:
        T, H = h.shape
        base = h.as_strided((max(T, 1), H + 8), (H + 8, 1)).to(device)
        h = base[:T, :H]
    mv = (lambda v: v.to(device)) if device is not None else (lambda v: v)
    return h, mv(p["cu"]), mv(p["pool_w"]), mv(p["pool_b"]), mv(p["cls_w"]), mv(p["cls_b"])


# ---- random inputs: fp64 evaluation of the same values and the error bound of the fp32 kernel
TAU = 4 * 2.0 ** -24  # error allowed to tanhf: ASSUMED 4 ulp of a value below 1 (docs/rerank.md)
SIG = 4 * 2.0 ** -24  # error allowed to the sigmoid on top of the logit's bound / 4


def random_head(H, B, seed=0, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    lens = [1 + (i * 5) % 7 for i in range(B)]
    T = sum(lens)
    base = torch.randn(T, H + 8, generator=g).to(dtype)
    cu = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32)
    return dict(hidden=base[:, :H], cu=cu,
                pool_w=(torch.randn(H, H, generator=g) * 0.05).to(dtype),
                pool_b=(torch.randn(H, generator=g) * 0.02).to(dtype),
                cls_w=(torch.randn(1, H, generator=g) * 0.05).to(dtype),
                cls_b=torch.tensor([0.01]).to(dtype))


def head_fp64(hidden, cu, pool_w, pool_b, cls_w, cls_b):
    """-> (logits fp64 [B], bound [B]) for the given (bf16 / f32) values:
    |ds| <= sum_j |c_j| (2 H 2^-24 (sum_k |w_jk x_k| + |b_j|) + TAU) + 2 H 2^-24 sum_j |c_j|
    (the fp32 dot's rounding through the 1-Lipschitz tanh, tanhf's own error, the final sum)."""
    cu = [int(v) for v in cu]
    H = hidden.shape[1]
    W = pool_w.detach().cpu().double().numpy()
    pb = pool_b.detach().cpu().double().numpy() if pool_b is not None else np.zeros(H)
    c = cls_w.detach().cpu().double().numpy().reshape(-1)
    cb = float(cls_b.detach().cpu().double().reshape(-1)[0]) if cls_b is not None else 0.0
    u = 2.0 * H * 2.0 ** -24
    s, bound = [], []
    for b in range(len(cu) - 1):
        x = hidden[cu[b]].detach().cpu().double().numpy() if cu[b + 1] > cu[b] else np.zeros(H)
        a = W @ x + pb
        s.append(float(np.tanh(a) @ c + cb))
        mag = np.abs(W) @ np.abs(x) + np.abs(pb)
        bound.append(float(np.sum(np.abs(c) * (u * mag + TAU)) + u * np.sum(np.abs(c))))
    return np.array(s), np.array(bound)


PAIR_QUERY = "how do I scale the echoserver deployment when the queue grows"
PAIR_DOCS = [
    "Scale the deployment with kubectl scale --replicas once the queue depth passes the threshold.",
    "Logs of a crashed pod are read with kubectl logs --previous.",
    "short",
    "The scaling runbook: check CPU saturation, then the HPA's target, then scale by one step. " * 6,
    "namespaces dev and staging allow restarts",
    "",
    "Restart a deployment with kubectl rollout restart; wait for the rollout to finish.",
    "A readiness probe that fails keeps the pod out of the service's endpoints.",
    "Queue depth is exported as a custom metric by the echoserver sidecar.",
    "scale",
    "Evidence for a scale action must cite a runbook section with a cosine of at least 0.35.",
    "Minikube's ingress addon exposes the echoserver on port 8080 of the node.",
    "Rolling back: kubectl rollout undo deployment/echoserver.",
    "The agent refuses actions outside the allowed namespaces.",
    "Replica counts above ten need a human's approval in this cluster.",
    "When the queue grows faster than the consumers drain it, add replicas; when it is flat, do nothing.",
]
