"""Plain-PyTorch fp32 reference implementations of every HIP kernel.

They define the numerics the kernels are tested against (tests compare the HIP op
with these on the same inputs) and they are the compute path for CPU runs (the
"Minimal_RAG on CPU" configuration).  Layouts match the kernels exactly:

* paged KV cache: ``[num_blocks, Hkv, block_size, D]``; ``slot = block * BS + off``
* packed QKV rows: ``[T, (Hq + 2*Hkv) * D]``
* cos/sin table: ``[max_pos, D]`` f32 = ``[cos(D/2) | sin(D/2)]``
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F


def rmsnorm(x, w, eps, residual=None):
    if residual is not None:
        s = (x.float() + residual.float()).to(x.dtype)
        residual.copy_(s)
        x = s
    xf = x.float()
    inv = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return ((xf * inv).to(x.dtype).float() * w.float()).to(x.dtype)


def layernorm(x, w, b, eps, residual=None, write_residual=False):
    if residual is not None:
        s = (x.float() + residual.float()).to(x.dtype)
        if write_residual:
            residual.copy_(s)
        x = s
    y = F.layer_norm(x.float(), (x.shape[-1],), w.float(), None if b is None else b.float(), eps)
    return y.to(x.dtype)


def embed_layernorm(ids, pos_ids, type_ids, tok, pos, typ, w, b, eps):
    e = tok[ids.long()].float()
    if pos is not None:
        e = e + pos[pos_ids.long()].float()
    if typ is not None:
        tid = type_ids.long() if type_ids is not None else torch.zeros_like(ids, dtype=torch.long)
        e = e + typ[tid].float()
    return F.layer_norm(e, (e.shape[-1],), w.float(), b.float(), eps).to(tok.dtype)


def silu_mul(x):
    i = x.shape[-1] // 2
    g, u = x[..., :i], x[..., i:]
    return (F.silu(g.float()).to(x.dtype).float() * u.float()).to(x.dtype)


def activation_(x, bias=None, kind=0):
    v = x.float()
    if bias is not None:
        v = (v + bias.float()).to(x.dtype).float()
    if kind == 0:
        v = F.gelu(v)
    elif kind == 1:
        v = F.gelu(v, approximate="tanh")
    else:
        v = F.relu(v)
    x.copy_(v.to(x.dtype))
    return x


def rope_cos_sin(max_pos, D, theta=10000.0, scaling=None, device=None):
    """[max_pos, D] f32 table = [cos | sin] over D/2 frequencies (neox convention).

    ``scaling``: dict for Llama-3.1 ``rope_type == "llama3"`` (factor, low_freq_factor,
    high_freq_factor, original_max_position_embeddings).
    """
    inv = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
    if scaling and scaling.get("rope_type", scaling.get("type")) == "llama3":
        factor = scaling["factor"]
        lf, hf = scaling["low_freq_factor"], scaling["high_freq_factor"]
        old = scaling["original_max_position_embeddings"]
        low_wl, high_wl = old / lf, old / hf
        wl = 2 * math.pi / inv
        smooth = (old / wl - lf) / (hf - lf)
        scaled = torch.where(wl > low_wl, inv / factor, inv)
        mid = (1 - smooth) * inv / factor + smooth * inv
        is_mid = (wl <= low_wl) & (wl >= high_wl)
        inv = torch.where(is_mid, mid, scaled)
    t = torch.arange(max_pos, dtype=torch.float64)
    f = torch.outer(t, inv)
    return torch.cat([f.cos(), f.sin()], dim=-1).float().to(device)


def _rotate(x, cs, neox):
    # x [T, H, D] f32; cs [T, D]
    D = x.shape[-1]
    c, s = cs[:, None, : D // 2], cs[:, None, D // 2:]
    if neox:
        x1, x2 = x[..., : D // 2], x[..., D // 2:]
        return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)
    x1, x2 = x[..., 0::2], x[..., 1::2]
    y = torch.empty_like(x)
    y[..., 0::2] = x1 * c - x2 * s
    y[..., 1::2] = x2 * c + x1 * s
    return y


def rope_kv_(qkv, positions, cos_sin, Hq, Hkv, D, k_cache=None, v_cache=None, slots=None,
             neox=True, write_k_inplace=False):
    T = qkv.shape[0]
    cs = cos_sin[positions.long()]
    q = qkv[:, : Hq * D].reshape(T, Hq, D)
    k = qkv[:, Hq * D:(Hq + Hkv) * D].reshape(T, Hkv, D)
    v = qkv[:, (Hq + Hkv) * D:(Hq + 2 * Hkv) * D].reshape(T, Hkv, D)
    qr = _rotate(q.float(), cs, neox).to(qkv.dtype)
    kr = _rotate(k.float(), cs, neox).to(qkv.dtype)
    qkv[:, : Hq * D] = qr.reshape(T, Hq * D)
    if write_k_inplace:
        qkv[:, Hq * D:(Hq + Hkv) * D] = kr.reshape(T, Hkv * D)
    if k_cache is not None:
        kv_write(kr, v, k_cache, v_cache, slots)
    return qkv


def kv_write(k, v, k_cache, v_cache, slots):
    BS = k_cache.shape[2]
    sl = slots.long()
    keep = sl >= 0
    sl = sl[keep]
    blk, off = sl // BS, sl % BS
    k_cache[blk, :, off] = k[keep].to(k_cache.dtype)
    v_cache[blk, :, off] = v[keep].to(v_cache.dtype)


def gather_paged(cache, block_table, n):
    """Rows 0..n-1 of one sequence from a paged cache -> [n, Hkv, D]."""
    BS = cache.shape[2]
    idx = torch.arange(n, device=cache.device)
    blk = block_table.long()[idx // BS]
    return cache[blk, :, idx % BS]


def attention_ref(q, k, v, causal, past=0, scale=None):
    """q [Sq, Hq, D], k/v [Sk, Hkv, D] -> [Sq, Hq, D] (GQA by head repetition)."""
    Sq, Hq, D = q.shape
    Sk, Hkv, _ = k.shape
    g = Hq // Hkv
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    kf = k.float().repeat_interleave(g, dim=1)
    vf = v.float().repeat_interleave(g, dim=1)
    s = torch.einsum("qhd,khd->hqk", q.float(), kf) * scale
    if causal:
        qpos = past + torch.arange(Sq, device=q.device)[:, None]
        kpos = torch.arange(Sk, device=q.device)[None, :]
        s = s.masked_fill((kpos > qpos)[None], float("-inf"))
    p = torch.softmax(s, dim=-1)
    return torch.einsum("hqk,khd->qhd", p, vf)


def paged_decode(q, k_cache, v_cache, block_tables, ctx_lens, scale):
    B, Hq, D = q.shape
    out = torch.empty_like(q)
    for b in range(B):
        n = int(ctx_lens[b])
        k = gather_paged(k_cache, block_tables[b], n)
        v = gather_paged(v_cache, block_tables[b], n)
        out[b] = attention_ref(q[b:b + 1], k, v, False, scale=scale)[0].to(q.dtype)
    return out


def attention_partials(q, k, v, causal, past=0, scale=None):
    """Unnormalised attention of q [Sq, Hq, D] over k/v [Sk, Hkv, D] in the format of the flash
    kernel's partial mode: (o f32 [Sq, Hq, D] = sum_j 2^(s_j - m) v_j, m f32 [Sq, Hq] = the row
    max of the scores in the log2 domain, l f32 [Sq, Hq] = sum_j 2^(s_j - m)).  A row that sees
    no key (``past`` may be negative) has o = 0, m = -inf, l = 0."""
    Sq, Hq, D = q.shape
    Sk, Hkv, _ = k.shape
    g = Hq // Hkv
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    kf = k.double().repeat_interleave(g, dim=1)
    vf = v.double().repeat_interleave(g, dim=1)
    s = torch.einsum("qhd,khd->hqk", q.double(), kf) * (scale * 1.4426950408889634)
    if causal:
        qpos = past + torch.arange(Sq, device=q.device)[:, None]
        kpos = torch.arange(Sk, device=q.device)[None, :]
        s = s.masked_fill((kpos > qpos)[None], float("-inf"))
    if Sk:
        m = s.amax(dim=-1)
    else:
        m = torch.full((Hq, Sq), float("-inf"), dtype=torch.float64, device=q.device)
    p = torch.exp2(s - torch.where(torch.isinf(m), torch.zeros_like(m), m)[..., None])
    o = torch.einsum("hqk,khd->qhd", p, vf)
    return o.float(), m.T.float(), p.sum(dim=-1).T.float()


def flash_prefill(q, k, v, block_tables, cu_q, ctx_lens, Hq, Hkv, D, scale, causal, q_past=None,
                  partials=False):
    """q [T, >=Hq*D]; paged (block_tables given) or dense k/v [T, >=Hkv*D].  ``q_past`` [B]:
    position of each sequence's first query relative to its first key for the causal mask
    (default ctx_len - q_len).  ``partials``: return the unnormalised (o f32 [T, Hq, D],
    m f32 [T, Hq], l f32 [T, Hq]) of :func:`attention_partials` instead of the bf16 output,
    whose rows without a visible key are zero."""
    T = q.shape[0]
    out = torch.zeros(T, Hq * D, dtype=q.dtype, device=q.device)
    if partials:
        po = torch.zeros(T, Hq, D, dtype=torch.float32, device=q.device)
        pm = torch.full((T, Hq), float("-inf"), dtype=torch.float32, device=q.device)
        pl = torch.zeros(T, Hq, dtype=torch.float32, device=q.device)
    cu = [int(x) for x in cu_q]
    for b in range(len(cu) - 1):
        s, e = cu[b], cu[b + 1]
        if e == s:
            continue
        qb = q[s:e, : Hq * D].reshape(e - s, Hq, D)
        if block_tables is not None:
            n = int(ctx_lens[b])
            kb = gather_paged(k, block_tables[b], n)
            vb = gather_paged(v, block_tables[b], n)
        else:
            n = e - s
            kb = k[s:e, : Hkv * D].reshape(n, Hkv, D)
            vb = v[s:e, : Hkv * D].reshape(n, Hkv, D)
        past = int(q_past[b]) if q_past is not None else n - (e - s)
        if partials or q_past is not None:
            o, m, l = attention_partials(qb, kb, vb, causal, past=past, scale=scale)
            if partials:
                po[s:e], pm[s:e], pl[s:e] = o, m, l
                continue
            o = o / l.clamp_min(1e-30)[..., None]  # rows without a visible key: 0 / tiny = 0
        else:
            o = attention_ref(qb, kb, vb, causal, past=past, scale=scale)
        out[s:e] = o.reshape(e - s, Hq * D).to(q.dtype)
    return (po, pm, pl) if partials else out


def cosine_scores(corpus, cnorm, queries, qnorm, eps=1e-9):
    dot = queries.double() @ corpus.double().T
    return dot / (qnorm.double()[:, None] * cnorm.double()[None, :] + eps)


def stable_topk(scores, K):
    """Descending scores, ties by ascending index (C# OrderByDescending is stable).  A NaN score is
    absent, as in the kernels (where NaN is never better than anything): the row is left out and
    (-inf, -1) pads follow."""
    nq, N = scores.shape
    out_s = torch.full((nq, K), float("-inf"), dtype=torch.float32)
    out_i = torch.full((nq, K), -1, dtype=torch.int32)
    for i in range(nq):
        row = scores[i].tolist()
        order = sorted((j for j in range(N) if row[j] == row[j]), key=lambda j: (-row[j], j))[:K]
        out_i[i, : len(order)] = torch.tensor(order, dtype=torch.int32)
        out_s[i, : len(order)] = scores[i, order].float()
    return out_s, out_i


def knn_merge(cand_s, cand_i, K):
    """The K best of each row's (score, id) candidates, (score desc, id asc); a candidate with
    id < 0 or a NaN score is absent, (-inf, -1) pads follow."""
    nq = cand_s.shape[0]
    out_s = torch.full((nq, K), float("-inf"))
    out_i = torch.full((nq, K), -1, dtype=torch.int32)
    for r in range(nq):
        pairs = [(s, i) for s, i in zip(cand_s[r].tolist(), cand_i[r].tolist()) if i >= 0 and s == s]
        pairs.sort(key=lambda p: (-p[0], p[1]))
        for j, (s, i) in enumerate(pairs[:K]):
            out_s[r, j] = s
            out_i[r, j] = i
    return out_s, out_i


def knn_topk(corpus, cnorm, queries, qnorm, K):
    sc = cosine_scores(corpus.float().cpu(), cnorm.cpu(), queries.float().cpu(), qnorm.cpu())
    return stable_topk(sc, K)


BM25_CHUNK = 4096     # csrc/kernels.h kLkBm25Chunk (the reference has no chunks; exported for the tests)
BM25_MAX_TERMS = 64   # csrc/kernels.h kLkBm25MaxTerms


def bm25_topk(term_ptr, post_doc, post_tf, kn, q_ptr, q_term, q_w, K):
    """fp32, in the kernel's operation order: per query, over its terms as given (ascending ids),
    ``score[d] += w_t * (tf / (tf + kn[d]))`` for every posting (d, tf) of the term -- the quotient,
    the product and the add each rounded to f32 -- then the documents with score > 0 ordered by
    (score desc, id asc); (-inf, -1) pads.  The index is CSR by term: ``term_ptr`` int64 [V+1],
    ``post_doc`` int32 [nnz] strictly ascending inside a term, ``post_tf`` uint8 [nnz], ``kn`` f32
    [N]; the queries ``q_ptr`` int32 [nq+1], ``q_term`` int32 / ``q_w`` f32 [nt]."""
    import numpy as np

    K = int(K)
    tp = term_ptr.cpu().numpy().astype(np.int64)
    pd = post_doc.cpu().numpy().astype(np.int64)
    tf = post_tf.cpu().numpy().astype(np.float32)
    knv = kn.cpu().numpy().astype(np.float32)
    qp = q_ptr.cpu().numpy().astype(np.int64)
    qt = q_term.cpu().numpy().astype(np.int64)
    qw = q_w.cpu().numpy().astype(np.float32)
    N, nq, V = len(knv), len(qp) - 1, len(tp) - 1
    if len(qt) != len(qw) or nq < 0 or qp[0] != 0 or qp[-1] != len(qt) or np.any(np.diff(qp) < 0):
        raise ValueError(f"bm25_topk: q_ptr must run from 0 to the number of query terms ({len(qt)})")
    if not 1 <= K <= 64:
        raise ValueError(f"bm25_topk: K must be in [1, 64] (got {K})")
    if nq and int(np.diff(qp).max()) > BM25_MAX_TERMS:
        raise ValueError(f"bm25_topk: a query has more than {BM25_MAX_TERMS} terms")
    out_s = np.full((nq, K), -np.inf, dtype=np.float32)
    out_i = np.full((nq, K), -1, dtype=np.int32)
    for q in range(nq):
        sc = np.zeros(N, dtype=np.float32)
        for j in range(qp[q], qp[q + 1]):
            t = qt[j]
            if not 0 <= t < V:
                continue
            d = pd[tp[t]:tp[t + 1]]
            f = tf[tp[t]:tp[t + 1]]
            sc[d] = sc[d] + qw[j] * (f / (f + knv[d]))  # a document appears once per term: no lost update
        hit = np.flatnonzero(sc > 0)
        order = hit[np.lexsort((hit, -sc[hit]))][:K]
        out_s[q, :len(order)] = sc[order]
        out_i[q, :len(order)] = order
    return torch.from_numpy(out_s), torch.from_numpy(out_i)


MMR_MAX_CAND = 64     # csrc/kernels.h kLkMmrMaxCand


def mmr_check(corpus, cnorm, cand_id, rel, lam, K):
    """The limits of ``mmr_select`` (csrc/mmr.hip), each refused by the argument's name."""
    if corpus.dim() != 2 or corpus.dtype != torch.bfloat16:
        raise ValueError("mmr_select: corpus must be bfloat16 [N, D]")
    N, D = corpus.shape
    if cnorm.dtype != torch.float32 or tuple(cnorm.shape) != (N,):
        raise ValueError("mmr_select: cnorm must be float32 [N]")
    if cand_id.dtype != torch.int32:
        raise ValueError("mmr_select: cand_id must be int32")
    if rel.dtype != torch.float32:
        raise ValueError("mmr_select: rel must be float32")
    if cand_id.dim() != 2 or cand_id.shape != rel.shape:
        raise ValueError("mmr_select: cand_id and rel must have the same shape [nq, C]")
    C = cand_id.shape[1]
    if not 1 <= C <= MMR_MAX_CAND:
        raise ValueError(f"mmr_select: C (the width of cand_id) must be in [1, {MMR_MAX_CAND}] (got {C})")
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 1 <= K <= C:
        raise ValueError(f"mmr_select: K must be an integer in [1, C = {C}] (got {K!r})")
    if D % 16 or not 16 <= D <= 1024:
        raise ValueError(f"mmr_select: D must be a multiple of 16 in [16, 1024] (got {D})")
    if isinstance(lam, bool) or not isinstance(lam, (int, float, np.floating, np.integer)) or not 0.0 <= float(lam) <= 1.0:
        raise ValueError(f"mmr_select: lam must be a finite number in [0, 1] (got {lam!r})")
    if N >= 1 << 31:
        raise ValueError(f"mmr_select: N must be below 2^31 (got {N})")


def mmr_select(corpus, cnorm, cand_id, rel, lam, K):
    """fp32, in the kernel's operation order (csrc/mmr.hip, docs/mmr.md): candidate i of a row is
    present iff ``0 <= cand_id[i] < N`` and ``rel[i]`` is not NaN; ``sim(i, j) = dot(c_i, c_j) /
    (cnorm[id_i] * cnorm[id_j] + 1e-9)`` with a plain fp32 matmul of the bf16 rows; K greedy rounds of
    ``mmr_i = lam * rel_i - (1 - lam) * m_i`` -- the two products and the difference each rounded to
    f32, ``1 - lam`` formed in f32 -- where ``m_i`` is 0 in round 0 and afterwards the largest
    similarity to a pick (assigned from the first pick); the pick is the present, not yet selected
    candidate with the largest mmr, ties to the lower position; a NaN mmr is not picked.
    -> (pos int32, ids int32, rel f32, mmr f32, max_sim f32), each [nq, K]; pads (-1, -1, -inf, -inf, -inf)."""
    mmr_check(corpus, cnorm, cand_id, rel, lam, K)
    K = int(K)
    X = corpus.float().cpu().numpy()
    cn = cnorm.cpu().numpy().astype(np.float32)
    cid = cand_id.cpu().numpy()
    rl = rel.cpu().numpy().astype(np.float32)
    N = X.shape[0]
    nq, C = cid.shape
    lam32 = np.float32(lam)
    oml = np.float32(1.0) - lam32
    o_pos = np.full((nq, K), -1, np.int32)
    o_id = np.full((nq, K), -1, np.int32)
    o_rel = np.full((nq, K), -np.inf, np.float32)
    o_mmr = np.full((nq, K), -np.inf, np.float32)
    o_sim = np.full((nq, K), -np.inf, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for q in range(nq):
            inside = (cid[q] >= 0) & (cid[q] < N)
            avail = inside & ~np.isnan(rl[q])
            if not avail.any():
                continue
            cl = np.where(inside, cid[q], 0)
            rows = X[cl]
            c = np.where(inside, cn[cl], np.float32(1.0)).astype(np.float32)
            den = (c[:, None] * c[None, :]).astype(np.float32) + np.float32(1e-9)
            S = ((rows @ rows.T).astype(np.float32) / den).astype(np.float32)
            lr = (lam32 * rl[q]).astype(np.float32)
            m = np.zeros(C, np.float32)
            for r in range(K):
                v = (lr - (oml * m).astype(np.float32)).astype(np.float32)
                ok = avail & ~np.isnan(v)
                if not ok.any():
                    break
                p = int(np.lexsort((np.arange(C), -np.where(ok, v, -np.inf), ~ok))[0])
                o_pos[q, r], o_id[q, r], o_rel[q, r], o_mmr[q, r], o_sim[q, r] = p, cid[q, p], rl[q, p], v[p], m[p]
                avail[p] = False
                m = S[:, p].copy() if r == 0 else np.where(S[:, p] > m, S[:, p], m)
    return tuple(torch.from_numpy(a) for a in (o_pos, o_id, o_rel, o_mmr, o_sim))


def pool_normalize(hidden, cu, mode, normalize):
    """An empty sequence (cu[b] == cu[b + 1]) pools to zeros, as the kernel writes them."""
    cu = [int(x) for x in cu]
    outs = []
    for b in range(len(cu) - 1):
        h = hidden[cu[b]:cu[b + 1]].float()
        if h.shape[0] == 0:
            outs.append(h.new_zeros(hidden.shape[1]))
            continue
        v = h[0] if mode == 1 else h.mean(0)
        if normalize:
            v = v / v.norm().clamp_min(1e-12)
        outs.append(v)
    return torch.stack(outs) if outs else hidden.new_zeros((0, hidden.shape[1]), dtype=torch.float32)


def rerank_head(hidden, cu, pool_w, pool_b, cls_w, cls_b, activation=0):
    """fp32, in the kernel's operation order: x = first row of each sequence (zeros if it is empty);
    a = pool_w x + pool_b; s = tanh(a) . cls_w + cls_b; out = sigmoid(s) if activation else s."""
    cu = [int(v) for v in cu]
    H = hidden.shape[1]
    W = pool_w.float().cpu()
    c = cls_w.float().cpu().reshape(-1)
    outs = []
    for b in range(len(cu) - 1):
        x = hidden[cu[b]].float().cpu() if cu[b + 1] > cu[b] else torch.zeros(H)
        a = (W * x[None, :]).sum(-1)
        if pool_b is not None:
            a = a + pool_b.float().cpu()
        s = (torch.tanh(a) * c).sum()
        if cls_b is not None:
            s = s + cls_b.float().cpu().reshape(())
        outs.append(1.0 / (1.0 + torch.exp(-s)) if activation else s)
    out = torch.stack(outs) if outs else torch.zeros(0)
    return out.to(torch.float32).to(hidden.device)


def row_norms(x):
    return x.float().norm(dim=-1)


def select_tokens(logits, temps=None, seed=0, step=0):
    if temps is None:
        return logits.float().argmax(-1).int()
    out = []
    g = torch.Generator(device="cpu").manual_seed(int(seed) * 1000003 + int(step))
    for i in range(logits.shape[0]):
        t = float(temps[i])
        row = logits[i].float().cpu()
        if t <= 0:
            out.append(int(row.argmax()))
        else:
            u = torch.rand(row.shape, generator=g).clamp(1e-12, 1 - 1e-7)
            out.append(int((row / t - torch.log(-torch.log(u))).argmax()))
    return torch.tensor(out, dtype=torch.int32, device=logits.device)


def argmax_key(logits, vocab_lo: int = 0):
    """Order-preserving int64 (max value, ~(vocab_lo + first argmax)) key per row (the HIP
    kernel's encoding: csrc/sampling.hip select_kernel<..., KEY>)."""
    x = logits.float()
    x = torch.where(torch.isnan(x), torch.full_like(x, float("-inf")), x)  # NaN counts as -inf
    idx = x.argmax(-1)
    best = x.gather(1, idx[:, None]).squeeze(1)
    best = torch.where(best == 0, torch.zeros_like(best), best)  # -0.0 is keyed as +0.0: they compare equal
    fb = best.view(torch.int32).long() & 0xFFFFFFFF
    u = torch.where(fb >= 0x80000000, (~fb) & 0xFFFFFFFF, fb | 0x80000000)
    hi = (u ^ 0x80000000) - ((u ^ 0x80000000) >= 0x80000000).long() * (1 << 32)  # signed 32-bit
    lo = (~(idx + vocab_lo)) & 0xFFFFFFFF
    return hi * (1 << 32) + lo


def keys_to_ids(keys):
    k = keys.max(dim=0).values
    return ((~(k & 0xFFFFFFFF)) & 0xFFFFFFFF).int()


LOGPROBS_MAX_N = 20  # csrc/sampling.hip kLpMaxN


def token_logprobs(logits, ids, rows, n: int):
    """fp32 reference of lk_token_logprobs (csrc/sampling.hip): for each requesting batch row
    ``rows[r]``, ``log_softmax`` of its logits as stored at ``ids[rows[r]]`` -> chosen_lp f32
    [R], and at the ``min(n, V)`` most likely ids ordered by (value desc, id asc) -> top_lp f32
    [R, n'], top_id int32 [R, n'].  The logits are not modified."""
    if not 0 <= int(n) <= LOGPROBS_MAX_N:
        raise ValueError(f"token_logprobs: n must be in 0..{LOGPROBS_MAX_N}, got {n}")
    V = logits.shape[1]
    ne = min(int(n), V)
    rows_l = rows.long()
    x = logits.index_select(0, rows_l).float()
    lp = torch.log_softmax(x, dim=-1)
    chosen = lp.gather(1, ids.long().index_select(0, rows_l)[:, None]).squeeze(1)
    order = torch.sort(x, dim=-1, descending=True, stable=True).indices[:, :ne]
    return chosen, lp.gather(1, order), order.int()


def mask_logits(logits, pool, mask_row, out=None):
    """fp32 reference of lk_mask_logits (csrc/token_mask.hip): ``out[b, v] = f32(logits[b, v])``
    (bit-exact) where ``mask_row[b] < 0`` or bit ``v & 31`` of ``pool[mask_row[b], v >> 5]`` is
    set, else ``-inf``; a ``mask_row[b] >= R`` masks the whole row.  ``pool`` int32 [R, words]
    with ``words == ceil(V / 32)`` (anything else raises); ``out``: optional f32 [B, V] view."""
    B, V = logits.shape
    R, words = pool.shape
    if words != (V + 31) // 32:
        raise ValueError(f"mask_logits: pool rows of {words} words for V = {V} (need {(V + 31) // 32})")
    mr = mask_row[:B].long()
    v = torch.arange(V, device=logits.device)
    if R > 0:
        w = pool.index_select(0, mr.clamp(0, R - 1))[:, v >> 5]
        bit = ((w >> (v & 31).to(w.dtype)[None]) & 1) != 0
    else:
        bit = torch.zeros((B, V), dtype=torch.bool, device=logits.device)
    keep = (bit & (mr < R)[:, None]) | (mr < 0)[:, None]
    res = torch.where(keep, logits.float(), torch.full((), float("-inf"), device=logits.device))
    if out is None:
        return res
    out.copy_(res)
    return out


def repeat_penalty_(logits, window, penalty):
    for b in range(logits.shape[0]):
        p = float(penalty[b])
        toks = sorted({int(t) for t in window[b].tolist() if int(t) >= 0})
        if not toks:
            continue
        idx = torch.tensor(toks, device=logits.device)
        l = logits[b, idx].float()
        logits[b, idx] = torch.where(l > 0, l / p, l * p).to(logits.dtype)
    return logits


SAMPLE_KMAX = 1024  # csrc/sampling.hip kSampKMax


def sample(logits, prm, hist, hist_len, seed=0, bias=None):
    """fp32 reference of lk_sample (csrc/sampling.hip), rows [B, 8] or [B, 12]: per row the
    logit bias (``bias``: int32 CSR [B+1 offsets | n ids | n f32 bits], ids outside [0, V)
    ignored), then over the last min(len, last_n) ring entries each unique token t with c
    occurrences gets l[t] = rp(l[t]) - (c * frequency + presence) (rp: the repeat penalty),
    top-k by (value desc, index asc), softmax at the row's temperature, the top-p prefix (a
    token is kept while the mass before it is <= top_p) cut further to the min-p prefix
    (p_i >= min_p * p_0), one draw; the token is appended to the ring.  Same distribution as
    the kernel (the random stream differs: torch's generator seeded per (seed, request seed,
    position))."""
    B, V = logits.shape
    W = hist.shape[1]
    out = torch.empty(B, dtype=torch.int32)
    P = prm.cpu()
    if P.dim() != 2 or P.shape[0] != B or P.shape[1] not in (8, 12):
        raise ValueError("prm [B, 8] or [B, 12]")
    wide = P.shape[1] == 12
    f32 = torch.float32
    C = None
    if bias is not None:
        C = bias.cpu()
        if C.dtype != torch.int32 or C.dim() != 1 or C.numel() < B + 1 or C.numel() != B + 1 + 2 * int(C[B]):
            raise ValueError("bias int32 [B+1 offsets | n ids | n values]")
    for r in range(B):
        row = P[r]
        temp = float(row[0:1].view(torch.float32)[0])
        top_p = float(row[1:2].view(torch.float32)[0])
        pen = float(row[2:3].view(torch.float32)[0])
        top_k, last_n, slot, reset, rseed = (int(x) for x in row[3:8])
        min_p, presence, frequency = (float(row[i:i + 1].view(f32)[0]) for i in (8, 9, 10)) if wide else (0.0, 0.0, 0.0)
        hl = 0 if reset else int(hist_len[slot])
        l = logits[r].float().clone()
        edited = False
        if C is not None and int(C[r + 1]) > int(C[r]):
            nb = int(C[B])
            for j in range(int(C[r]), int(C[r + 1])):
                t = int(C[B + 1 + j])
                if 0 <= t < V:
                    l[t] = l[t] + C[B + 1 + nb + j: B + 2 + nb + j].view(f32)[0]
            edited = True
        if (pen != 1.0 or presence != 0.0 or frequency != 0.0) and last_n != 0:
            n = min(hl, last_n if last_n > 0 else W, W)
            count: dict = {}
            for j in range(n):
                t = int(hist[slot, (hl - 1 - j) % W])
                if 0 <= t < V:
                    count[t] = count.get(t, 0) + 1
            for t, c in count.items():
                x = l[t] / pen if l[t] > 0 else l[t] * pen
                if presence != 0.0 or frequency != 0.0:
                    x = x - (torch.tensor(float(c), dtype=f32) * torch.tensor(frequency, dtype=f32)
                             + torch.tensor(presence, dtype=f32))
                l[t] = x
            edited = True
        if edited:
            logits[r] = l.to(logits.dtype)
        greedy = temp <= 0.0
        K = 1 if greedy else min(top_k if top_k > 0 else SAMPLE_KMAX, V, SAMPLE_KMAX)
        order = _topk_stable(l, K)
        if greedy or K == 1:
            tok = order[0]
        else:
            v = l[torch.tensor(order)].double()
            e = torch.exp((v - v[0]) / temp)
            incl = torch.cumsum(e, 0)
            keep = (incl - e) <= top_p * incl[-1]
            if min_p > 0.0:
                keep &= e >= min_p
                keep[0] = True
            nkeep = int(keep.sum())
            g = torch.Generator().manual_seed((int(seed) * 1000003 + rseed * 7919 + hl) & ((1 << 62) - 1))
            u = float(torch.rand((), generator=g, dtype=torch.float64)) * float(incl[nkeep - 1])
            pick = int((incl[:nkeep] > u).nonzero()[0]) if bool((incl[:nkeep] > u).any()) else nkeep - 1
            tok = order[pick]
        out[r] = tok
        hist[slot, hl % W] = tok
        hist_len[slot] = hl + 1
    return out.to(logits.device)


def _topk_stable(l, K):
    """indices of the K largest (value desc, index asc)."""
    vals, idx = torch.sort(l, descending=True, stable=True)
    return idx[:K].tolist()


# ---------------------------------------------------------------- fused prefill chain
# (csrc/gemm.hip LkEpi: the decoder block's RMSNorm folded into its neighbouring GEMMs)
def ss_partials(r: torch.Tensor, cols: int = 256) -> torch.Tensor:
    """Per-``cols``-column partial sums of squares of r [M, N]: [N / cols, M] f32."""
    M, N = r.shape
    return r.float().pow(2).reshape(M, N // cols, cols).sum(-1).t().contiguous()


def row_scale(ss: torch.Tensor, H: int, eps: float) -> torch.Tensor:
    """[M] f32 rsqrt(mean of squares + eps) from the partials [nt, >= M]."""
    return torch.rsqrt(ss.float().sum(0) / H + eps)


def _mm(x, w):
    """x w^T in fp32: the product of the fused-chain oracles below (one place, so a test can pin
    its summation order per row: the library's depends on the number of rows)."""
    return x.float() @ w.float().t()


def linear_resid(x, w, residual, ss_out):
    """residual = bf16(residual + bf16(x w^T)) in place; ss_out [N/256, >= M] = its partials."""
    y = _mm(x, w).to(x.dtype)
    residual.copy_((residual.float() + y.float()).to(residual.dtype))
    M = residual.shape[0]
    ss_out[:, :M] = ss_partials(residual)
    return residual


def gemm_scaled(x, w, ss, H, eps, swiglu=False):
    """x w^T with each row scaled by the folded norm's rsqrt (ss None: unscaled); SwiGLU:
    silu(g) * u on the scaled, bf16-rounded halves."""
    acc = _mm(x, w)
    if ss is not None:
        acc = acc * row_scale(ss, H, eps)[: x.shape[0], None]
    if not swiglu:
        return acc.to(x.dtype)
    I = w.shape[0] // 2
    g, u = acc[:, :I].to(x.dtype).float(), acc[:, I:].to(x.dtype).float()
    return ((g * torch.sigmoid(g)).to(x.dtype).float() * u).to(x.dtype)


def qkv_fused(x, w, ss, H, eps, positions, cos_sin, Hq, Hkv, D, k_cache=None, v_cache=None, slots=None):
    """The QKV GEMM's fused epilogue: scaled, bf16-rounded projection, interleaved-pair RoPE on
    q and k (written back into the row), K / V into the paged cache."""
    qkv = gemm_scaled(x, w, ss, H, eps)
    return rope_kv_(qkv, positions, cos_sin, Hq, Hkv, D, k_cache, v_cache, slots, neox=False, write_k_inplace=True)


def gather_step(idx, x, x2=None, ss=None, pos=None, ss_ld=0, ss_out=None):
    """ops.gather_step: rows idx of x / x2, columns idx of the planes ss, pos[idx]."""
    i = idx.long()
    R = i.numel()
    ss_c = None
    if ss is not None:
        ss_c = ss_out if ss_out is not None else torch.zeros(ss.shape[0], max(ss_ld, R, 1), dtype=ss.dtype,
                                                             device=ss.device)
        ss_c[:, :R] = ss.index_select(1, i)
    return (x.index_select(0, i), None if x2 is None else x2.index_select(0, i), ss_c,
            None if pos is None else pos.index_select(0, i))
