"""Sampling parameters (Ollama ``options`` semantics) and the batched sampler.

Fast paths: an all-greedy batch is one HIP argmax kernel over the logits; a batch
with temperatures but no top-k/top-p/penalty is one HIP Gumbel-max kernel.  Anything
else -- Ollama's defaults (temperature 0.8, top-k 40, top-p 0.9, repeat penalty 1.1 over
the last 64 tokens, which is what an OllamaSharp client gets: it sends no options) -- is
``ops.sample``: two HIP launches (csrc/sampling.hip lk_sample) driven by one int32
parameter row per sequence, with each sequence's generated tokens kept in a device
history ring that the kernel itself appends to (the host never builds a penalty
window, and with pipelined steps the ring already holds the token the host has not
collected yet).  min_p, presence / frequency penalty and logit_bias (docs/sampling.md) run
in the same two launches: a batch that sets one of them uploads 12-wide rows and / or a
sparse bias operand, every other batch the 8-wide rows it always did.

Rows whose processor returns a ``TokenMask`` (JSON-schema decoding, docs/structured_outputs.md)
are constrained on the device: the masks live in a lazily created pool of bitmask rows, a step
uploads only the masks the pool does not hold plus one row index per batch row, and one
``ops.mask_logits`` launch writes the masked f32 copy of the logits that the batch's selector
then reads.  A batch without such a row runs the code it always did.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import Callable, Optional

import numpy as np
import torch

from .. import ops
from .schema_grammar import TokenMask


@dataclass
class SamplingParams:
    temperature: float = 0.8
    top_k: int = 40
    top_p: float = 0.9
    repeat_penalty: float = 1.1
    repeat_last_n: int = 64
    seed: Optional[int] = None
    max_tokens: int = 256
    min_tokens: int = 0
    stop: list = field(default_factory=list)
    ignore_eos: bool = False
    # callable(generated_ids) -> allowed token-id tensor/list or None (constrained decoding)
    logits_processor: Optional[Callable] = None
    # token log-probabilities of the model's own distribution (docs/logprobs.md): the chosen
    # token's, and the top_logprobs (0..20) most likely tokens' per generated token
    logprobs: bool = False
    top_logprobs: int = 0
    # sampler controls (docs/sampling.md): min_p keeps a candidate while p_i >= min_p * p_max;
    # presence / frequency are subtracted per unique token / per occurrence in the repeat window;
    # logit_bias {token id: f32} is added to the logits before anything else
    min_p: float = 0.0
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    logit_bias: Optional[dict] = None

    def __post_init__(self):
        if self.logit_bias is not None and not isinstance(self.logit_bias, dict):
            # the wire form (msgpack has no integer-keyed maps in strict mode): [[id, value], ...]
            self.logit_bias = {int(k): float(v) for k, v in self.logit_bias}
        if not self.logit_bias:
            self.logit_bias = None

    @classmethod
    def greedy(cls, max_tokens: int = 256, **kw) -> "SamplingParams":
        return cls(temperature=0.0, top_k=0, top_p=1.0, repeat_penalty=1.0, max_tokens=max_tokens, **kw)

    @classmethod
    def from_ollama(cls, options: Optional[dict], defaults=None, num_predict_default: int = 256) -> "SamplingParams":
        """Map an Ollama ``options`` dict (temperature, top_k, top_p, min_p, repeat_penalty,
        repeat_last_n, presence_penalty, frequency_penalty, seed, num_predict, stop) onto
        SamplingParams."""
        o = dict(options or {})
        d = defaults
        sp = cls(
            temperature=float(o.get("temperature", d.temperature if d else 0.8)),
            top_k=int(o.get("top_k", d.top_k if d else 40)),
            top_p=float(o.get("top_p", d.top_p if d else 0.9)),
            repeat_penalty=float(o.get("repeat_penalty", d.repeat_penalty if d else 1.1)),
            repeat_last_n=int(o.get("repeat_last_n", d.repeat_last_n if d else 64)),
            seed=o.get("seed"),
            min_p=float(o.get("min_p", 0.0)),
            presence_penalty=float(o.get("presence_penalty", 0.0)),
            frequency_penalty=float(o.get("frequency_penalty", 0.0)),
        )
        n = int(o.get("num_predict", d.num_predict if d else -1))
        sp.max_tokens = num_predict_default if n is None or n < 0 else n
        stop = o.get("stop") or []
        sp.stop = [stop] if isinstance(stop, str) else list(stop)
        return sp

    @property
    def is_greedy(self) -> bool:
        return self.temperature <= 0.0 or self.top_k == 1

    @property
    def reads_ring(self) -> bool:
        """A repeat, presence or frequency penalty reads the device history ring."""
        return self.repeat_last_n != 0 and (self.repeat_penalty != 1.0 or self.presence_penalty != 0.0
                                            or self.frequency_penalty != 0.0)


# grammar-constrained rows select over their allowed ids only (LK_SPARSE_SELECT=0: dense
# -inf mask over [rows, V] + full-row select, the path CPU tensors and top-k/top-p take)
SPARSE_SELECT = os.environ.get("LK_SPARSE_SELECT", "1") != "0"


class Sampler:
    def __init__(self, vocab_size: int, seed: int = 0, history_len: int = 256):
        self.vocab_size = vocab_size
        self.seed = seed
        # the device history ring holds a sequence's whole output (up to max_model_len), so
        # repeat_last_n > 256 and -1 (Ollama: the whole context) penalise the full history
        self.RING = max(256, -(-min(int(history_len), 32768) // 256) * 256)
        self.step = 0
        # processors return the same cached list objects for recurring grammar states:
        # memoise their int64 arrays (id -> (list, array); the list reference keeps the id valid)
        self._arr_cache: dict = {}

    def _as_array(self, allowed, V: int):
        """int64 array of the in-vocabulary ids of ``allowed`` (memoised for the recurring
        cached lists of a grammar)."""
        if isinstance(allowed, np.ndarray):
            a = allowed.astype(np.int64, copy=False)
            return a[(a >= 0) & (a < V)] if len(a) and (a.min() < 0 or a.max() >= V) else a
        hit = self._arr_cache.get(id(allowed))
        if hit is not None and hit[0] is allowed:
            return hit[1]
        a = np.asarray(allowed, dtype=np.int64)
        if len(a) and (a.min() < 0 or a.max() >= V):
            a = a[(a >= 0) & (a < V)]
        # every list, short ones too: the grammar states recur (literal / EOS lists)
        if len(self._arr_cache) > 8192:
            self._arr_cache.clear()
        self._arr_cache[id(allowed)] = (allowed, a)
        return a

    def _plan(self, rows: dict, B: int, dev) -> torch.Tensor:
        """Device int32 [B flags | B+1 offsets | allowed ids] of the constrained rows
        (flag 0 = unconstrained row) for the HIP select_allowed kernel.  Staged through a small
        ring of pinned buffers: a pageable host->device copy makes the host wait until the
        device queue reaches it (behind the step's forward), which would stall the pipelined
        engine's next launch."""
        order = sorted(rows)
        flags = np.zeros(B, dtype=np.int32)
        counts = np.zeros(B + 1, dtype=np.int64)
        for i in order:
            flags[i] = 1
            counts[i + 1] = len(rows[i])
        offs = np.cumsum(counts)
        ids = np.concatenate([rows[i] for i in order])
        plan = np.concatenate([flags, offs.astype(np.int32), ids.astype(np.int32)])
        return self._stage(plan, dev, "_plan")

    def _bias(self, params: list, V: int, dev) -> torch.Tensor:
        """Device int32 CSR [B+1 offsets | n ids | n f32 values as bits] of the rows' logit_bias
        (ids outside [0, V) dropped) for ops.sample; staged like :meth:`_plan`."""
        counts = np.zeros(len(params) + 1, dtype=np.int64)
        ids, vals = [], []
        for i, p in enumerate(params):
            if p.logit_bias:
                kept = [(int(t), float(v)) for t, v in p.logit_bias.items() if 0 <= int(t) < V]
                counts[i + 1] = len(kept)
                ids += [t for t, _ in kept]
                vals += [v for _, v in kept]
        csr = np.concatenate([np.cumsum(counts).astype(np.int32), np.asarray(ids, dtype=np.int32),
                              np.asarray(vals, dtype=np.float32).view(np.int32)])
        return self._stage(csr, dev, "_bias")

    def _stage(self, plan: np.ndarray, dev, name: str) -> torch.Tensor:
        """int32 host array -> device tensor through the small pinned ring ``name``."""
        if dev.type != "cuda":
            return torch.from_numpy(plan)
        src, slot = self._pinned(plan, name)
        out = torch.empty(plan.size, dtype=torch.int32, device=dev)
        out.copy_(src, non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record()
        return out

    def _pinned(self, plan: np.ndarray, name: str):
        """``plan`` copied into the next buffer of the pinned ring ``name`` -> (pinned view, ring
        slot); the caller records ``slot[1]`` behind its last copy out of the view."""
        ring = getattr(self, name + "_ring", None)
        if ring is None:
            ring = [[None, None] for _ in range(4)]  # [pinned int32 buffer, event]
            setattr(self, name + "_ring", ring)
            setattr(self, name + "_k", 0)
        k = (getattr(self, name + "_k") + 1) % len(ring)
        setattr(self, name + "_k", k)
        slot = ring[k]
        if slot[1] is not None:
            slot[1].synchronize()  # the copy that last read this buffer has run
        if slot[0] is None or slot[0].numel() < plan.size:
            slot[0] = torch.empty(max(2 * plan.size, 1 << 14), dtype=torch.int32, pin_memory=True)
        slot[0][: plan.size].numpy()[:] = plan
        return slot[0][: plan.size], slot

    # ---------------------------------------------------------------- device token-mask pool
    MASK_ROWS = 1024  # bitmask rows of the pool (16 MB at V = 128,256), LRU-evicted beyond

    def _mask_pool(self, dev, words: int) -> torch.Tensor:
        """int32 [MASK_ROWS, words] on ``dev``, created on the first TokenMask this sampler sees
        there (a server that never gets a schema allocates nothing)."""
        pool = getattr(self, "_mpool", None)
        if pool is None or pool.device != dev or pool.shape[1] != words:
            pool = self._mpool = torch.zeros((self.MASK_ROWS, words), dtype=torch.int32, device=dev)
            self._mrow_of: dict = {}  # id(mask) -> [mask, pool row, last step used] (the reference keeps the id valid)
            self._mfree = list(range(self.MASK_ROWS - 1, -1, -1))
        return pool

    def _mask_rows(self, masks: dict, B: int, V: int, dev):
        """(pool, device int32 [B] pool row per batch row, -1 = no mask) for the batch rows
        ``masks`` {row: TokenMask}.  Only masks the pool does not hold are uploaded: padded or
        truncated to ``V`` bits, staged through a pinned ring and copied into their rows without
        blocking -- stream order keeps a row that an earlier step still reads intact.  A new mask
        takes a free row or the least recently used one that this batch does not use."""
        words = (V + 31) // 32
        pool = self._mask_pool(dev, words)
        live = {id(m) for m in masks.values()}
        if len(live) > self.MASK_ROWS:
            raise RuntimeError(f"{len(live)} distinct token masks in one batch; the pool holds {self.MASK_ROWS}")
        mrow = np.full(B, -1, dtype=np.int32)
        new = []
        for i, m in masks.items():
            ent = self._mrow_of.get(id(m))
            if ent is None:
                if self._mfree:
                    row = self._mfree.pop()
                else:
                    victim = min((k for k in self._mrow_of if k not in live), key=lambda k: self._mrow_of[k][2])
                    row = self._mrow_of.pop(victim)[1]
                ent = self._mrow_of[id(m)] = [m, row, self.step]
                w = m.words[:words] if m.words.size >= words else np.concatenate(
                    [m.words, np.zeros(words - m.words.size, dtype=np.uint32)])
                new.append((row, w))
            ent[2] = self.step
            mrow[i] = ent[1]
        if new:
            host = np.concatenate([w for _, w in new]).view(np.int32)
            if dev.type != "cuda":
                src, slot = torch.from_numpy(host.copy()), None
            else:
                src, slot = self._pinned(host, "_mask")
            for j, (row, _) in enumerate(new):
                pool[row].copy_(src[j * words:(j + 1) * words], non_blocking=True)
            if slot is not None:
                slot[1] = torch.cuda.Event()
                slot[1].record()
        return pool, self._stage(mrow, dev, "_mrow")

    # ---------------------------------------------------------------- device sampler state
    RING = 256        # default history window per sequence (repeat_last_n is clamped to it)
    SLOTS = 1024      # sequences with a live ring (>= 2x max_num_seqs; LRU-evicted beyond)

    def _ring(self, dev):
        if getattr(self, "_hist", None) is None or self._hist.device != dev:
            self._hist = torch.zeros((self.SLOTS, self.RING), dtype=torch.int32, device=dev)
            self._hist_len = torch.zeros(self.SLOTS, dtype=torch.int32, device=dev)
            self._slot_of: dict = {}   # key -> (slot, request salt)
            self._lru: dict = {}       # key -> last step seen
            self._free = list(range(self.SLOTS - 1, -1, -1))
            self._assigned = 0
        return self._hist, self._hist_len

    def _slot(self, key, live: set):
        """(slot, reset, request salt) of sequence ``key``; a new key takes a free slot or,
        with none left, the least recently used one not in this batch."""
        hit = self._slot_of.get(key)
        if hit is not None:
            self._lru[key] = self.step
            return hit[0], 0, hit[1]
        if self._free:
            slot = self._free.pop()
        else:
            victim = min((k for k in self._lru if k not in live), key=self._lru.get)
            slot = self._slot_of.pop(victim)[0]
            self._lru.pop(victim)
        self._assigned += 1
        self._slot_of[key] = (slot, self._assigned)
        self._lru[key] = self.step
        return slot, 1, self._assigned

    def release(self, key):
        """Forget a finished sequence's ring (its slot is reused)."""
        hit = getattr(self, "_slot_of", {}).pop(key, None)
        if hit is not None:
            self._lru.pop(key, None)
            self._free.append(hit[0])

    def _device_sample(self, logits, params, keys):
        dev = logits.device
        hist, hist_len = self._ring(dev)
        B = logits.shape[0]
        # 12-wide rows (min_p, presence, frequency) and the bias operand only for a batch that
        # sets one of them: every other batch uploads the 8-wide rows it always did
        wide = any(p.min_p > 0.0 or p.presence_penalty != 0.0 or p.frequency_penalty != 0.0 for p in params)
        bias = self._bias(params, logits.shape[1], dev) if any(p.logit_bias for p in params) else None
        prm = np.zeros((B, 12 if wide else 8), dtype=np.int32)
        f = prm.view(np.float32)
        live = set(keys)
        seed = self.seed
        for i, (p, key) in enumerate(zip(params, keys)):
            slot, reset, salt = self._slot(key, live)
            f[i, 0] = 0.0 if p.is_greedy else p.temperature
            f[i, 1] = p.top_p
            f[i, 2] = p.repeat_penalty
            prm[i, 3] = p.top_k
            prm[i, 4] = min(p.repeat_last_n, self.RING) if p.repeat_last_n >= 0 else self.RING
            prm[i, 5] = slot
            prm[i, 6] = reset
            prm[i, 7] = (int(p.seed) if p.seed is not None else salt) & 0x7FFFFFFF
            if wide:
                f[i, 8], f[i, 9], f[i, 10] = p.min_p, p.presence_penalty, p.frequency_penalty
        prm_t = torch.from_numpy(prm)
        if dev.type == "cuda":
            prm_t = prm_t.pin_memory().to(dev, non_blocking=True)
        lg = logits if logits.dtype == torch.float32 and logits.is_contiguous() else logits.float().contiguous()
        if bias is None:
            return ops.sample(lg, prm_t, hist, hist_len, seed)
        return ops.sample(lg, prm_t, hist, hist_len, seed, bias=bias)

    # the last call's log-probabilities: None when no row asked, else (rows, n, chosen_lp [R],
    # top_lp [R, n'], top_id [R, n']) -- the requesting batch rows in order, the largest
    # top_logprobs among them, and ops.token_logprobs' tensors on the logits' device
    last_logprobs = None

    def __call__(self, logits: torch.Tensor, params: list, histories: list, keys: Optional[list] = None) -> torch.Tensor:
        """logits [B, V] (f32 or bf16) -> int32 token ids [B] (on logits.device).  ``keys``: a
        stable id per row's sequence (its history ring); default the row index.  When a row's
        params ask for ``logprobs``, the logits are left untouched (mask and penalty work on
        a private copy) and :attr:`last_logprobs` holds the result of one
        ``ops.token_logprobs`` launch over the requesting rows; otherwise it is None and the
        call is the one it always was (the logits may be edited in place)."""
        want = [i for i, p in enumerate(params) if p.logprobs]
        self.last_logprobs = None
        if not want:
            return self._choose(logits, params, histories, keys, False)
        ids = self._choose(logits, params, histories, keys, True)
        n = max(min(max(int(params[i].top_logprobs), 0), ops.ref.LOGPROBS_MAX_N) for i in want)
        rows_t = torch.tensor(want, dtype=torch.int32)
        if logits.device.type == "cuda":
            rows_t = rows_t.pin_memory().to(logits.device, non_blocking=True)
        ids32 = ids if ids.dtype == torch.int32 else ids.int()
        self.last_logprobs = (want, n) + tuple(ops.token_logprobs(logits, ids32, rows_t, n))
        return ids

    def _choose(self, logits: torch.Tensor, params: list, histories: list, keys: Optional[list], keep: bool) -> torch.Tensor:
        """Token ids of every row; ``keep``: the caller's logits must stay as they are."""
        self.step += 1
        B = logits.shape[0]
        dev = logits.device
        keys = list(keys) if keys is not None else list(range(B))
        # constrained decoding: on the GPU the select kernel scans only each row's allowed
        # ids (one host->device copy of the id lists); otherwise everything outside the
        # allowed set is masked -- one copy of the flat (row * V + token) positions and one
        # index_fill for the whole batch.  (An advanced-index assignment of a Python
        # scalar, mask[r, t] = 0.0, blocks the host until the device queue drains --
        # measured 15 ms behind a queued forward -- serialising the step pipelining.)
        V = logits.shape[1]
        rows, masks = {}, {}
        for i, p in enumerate(params):
            if p.logits_processor is not None:
                allowed = p.logits_processor(histories[i])
                if isinstance(allowed, TokenMask):
                    masks[i] = allowed
                elif allowed is not None:
                    rows[i] = self._as_array(allowed, V)
        if masks:
            # schema rows (docs/structured_outputs.md): one launch writes a private f32 copy of
            # the logits with every id outside a row's bitmask at -inf -- the copy the fused
            # sampler makes of bf16 logits anyway -- and the batch goes on to the selector it
            # would have used; rows with id lists are handled on that copy as they always were
            pool, mrow = self._mask_rows(masks, B, V, dev)
            logits = ops.mask_logits(logits, pool, mrow)
            keep = False  # the copy is ours to edit
        need_filter = any((not p.is_greedy) and (0 < p.top_k < V or p.top_p < 1.0 or p.min_p > 0.0) for p in params)
        need_penalty = any(p.reads_ring for p in params)
        need_bias = any(p.logit_bias for p in params)
        fused = need_filter or need_penalty or need_bias
        plan = None
        if rows and not fused and SPARSE_SELECT and ops.use_hip(logits):
            # selection straight over each row's allowed ids (HIP select_allowed): no mask
            plan = self._plan(rows, B, dev)
        if keep and ((rows and plan is None) or fused):
            # the dense mask and the penalty kernel edit their input: give them a private copy
            # (the f32 copy the fused sampler would make of bf16 logits anyway, else a clone)
            logits = logits.float().contiguous() if fused and logits.dtype != torch.float32 else logits.clone()
        if plan is None and rows:
            crow = list(rows)
            flat = [rows[i] + j * V for j, i in enumerate(crow)]
            idx = torch.from_numpy(np.concatenate(flat)).to(dev, non_blocking=True)
            mask = torch.full((len(crow), V), float("-inf"), device=dev, dtype=logits.dtype)
            mask.view(-1).index_fill_(0, idx, 0.0)
            sel = torch.from_numpy(np.asarray(crow, dtype=np.int64)).to(dev, non_blocking=True)
            logits.index_add_(0, sel, mask)
        if fused:
            # Ollama's chain (bias -> penalties -> top-k -> temperature -> top-p -> min-p -> draw)
            # in one fused kernel
            return self._device_sample(logits, params, keys)
        if all(p.is_greedy for p in params):
            if plan is not None:
                return ops.lib().select_allowed(logits, plan)
            return ops.select_tokens(logits)
        temps = torch.tensor([0.0 if p.is_greedy else p.temperature for p in params], dtype=torch.float32)
        seed = self.seed
        for p in params:
            if p.seed is not None:
                seed = int(p.seed)
                break
        if plan is not None:
            return ops.lib().select_allowed(logits, plan, temps.to(dev), seed, self.step)
        return ops.select_tokens(logits, temps.to(dev), seed=seed, step=self.step)
