"""Step shapes for the last-layer-rows tests (CPU reference ops and GPU kernels alike).

A step is built from real Sequence objects through the runner's own ``prepare`` / ``_meta``, over a
KV cache pre-filled with random finite values (the same in every run): the keys a row sees below
the step's own rows are that filling, so no set-up steps are needed and every slot the step does
not write must still hold it afterwards.  Plain torch, importable on the CPU; the tests import
this module as a sibling."""
import torch

from llm_kubernetes_minikube_sharp4dev_amd.engine.model_runner import ModelRunner
from llm_kubernetes_minikube_sharp4dev_amd.engine.sampling import SamplingParams
from llm_kubernetes_minikube_sharp4dev_amd.engine.sequence import Sequence
from llm_kubernetes_minikube_sharp4dev_amd.models import build_decoder
from llm_kubernetes_minikube_sharp4dev_amd.models.configs import DecoderConfig

BS = 16
VOCAB = 512
NUM_BLOCKS = 1024


def build_model(device, dtype=torch.bfloat16):
    """The smallest folded Llama the fused chain accepts: hidden 1024, 8 query heads x 128, 2 KV
    heads, intermediate 2048, 2 layers; random weights, non-unit norms folded in."""
    cfg = DecoderConfig("t", "llama", 2, 1024, 8, 2, 128, 2048, VOCAB, max_position=1024, rope_theta=10000.0)
    m = build_decoder(cfg, device=device, dtype=dtype).random_init(3)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for L in m.layers:
            for w in (L.input_norm, L.post_norm):
                w.copy_((torch.rand(w.shape, generator=g) * 1.5 + 0.25).to(w.dtype))
        m.final_norm.copy_((torch.rand(m.final_norm.shape, generator=g) * 1.5 + 0.25).to(m.final_norm.dtype))
    m.fold_norms()
    assert m.folded and not m.rope_neox
    return m


def new_runner(model, seed=7):
    """A runner whose whole cache holds random finite values (seeded: equal in every run)."""
    r = ModelRunner(model, block_size=BS, max_model_len=512, max_num_seqs=256, num_blocks=NUM_BLOCKS, use_graphs=False)
    g = torch.Generator().manual_seed(seed)
    fill = (torch.randn(r.kv.shape, generator=g, dtype=torch.float32) * 0.5).to(r.kv.dtype)
    r.kv.copy_(fill.to(r.kv.device))
    return r


class StepMaker:
    """Sequences over block tables of their own, taken in order from block 1 on."""

    def __init__(self, seed=5):
        self.next_block = 1
        self.gen = torch.Generator().manual_seed(seed)

    def _ids(self, n):
        return torch.randint(3, VOCAB, (n,), generator=self.gen).tolist()

    def _table(self, ntok):
        nb = (ntok + BS - 1) // BS
        t = list(range(self.next_block, self.next_block + nb))
        self.next_block += nb
        assert self.next_block <= NUM_BLOCKS
        return t

    def prefill(self, start, n, plen=None):
        """Rows [start, start + n) of a prompt of ``plen`` tokens (default: the chunk ends it); the
        positions below ``start`` count as computed (a prefix-cache hit or an earlier chunk)."""
        plen = start + n if plen is None else plen
        s = Sequence(self._ids(plen), SamplingParams(), block_table=self._table(max(plen, start + n + 1)), num_computed=start)
        return (s, start, n)

    def decode(self, ctx):
        """One decode row whose context, its own key included, is ``ctx`` keys."""
        st = ctx - 1
        s = Sequence(self._ids(st), SamplingParams(), output_ids=self._ids(1), block_table=self._table(ctx + 1),
                     num_computed=st)
        return (s, st, 1)

    def extend(self, start, n):
        """A jump-forward chunk: n host-appended output tokens after ``start`` computed ones."""
        s = Sequence(self._ids(start), SamplingParams(), output_ids=self._ids(n), block_table=self._table(start + n + 1),
                     num_computed=start)
        return (s, start, n)


def mixed_333(mk):
    """3 decode rows, one 3-row jump-forward chunk, two prompts that finish (97 rows; 130 rows
    behind a prefix-cache hit of 32 keys) and one 100-row chunk that does not finish: 333 rows,
    of which 3 + 1 + 2 = 6 feed the LM head."""
    return [mk.decode(40), mk.prefill(0, 97), mk.decode(17), mk.extend(50, 3), mk.prefill(32, 130),
            mk.prefill(0, 100, plen=150), mk.decode(129)]


def follow_up(items):
    """The step after ``mixed_333`` on the same sequences: every finished item decodes one more
    token, the unfinished chunk goes on -- each reads the last layer's K / V of the step before."""
    nxt = []
    for s, st, n in items:
        s.num_computed = st + n
        if s.num_computed < len(s.prompt_ids):
            nxt.append((s, s.num_computed, len(s.prompt_ids) - s.num_computed))
            continue
        s.output_ids = list(s.output_ids) + [7 + len(nxt)]
        nxt.append((s, s.num_computed, 1))
    return nxt


def two_tiles(mk):
    """130 decode rows plus a 200-row finishing prompt: 131 gathered rows, two 128-row tiles."""
    return [mk.decode(5 + (i * 7) % 60) for i in range(130)] + [mk.prefill(0, 200)]


def no_logit_rows(mk):
    """Two unfinished chunks, 300 rows, nothing for the LM head."""
    return [mk.prefill(0, 180, plen=400), mk.prefill(48, 120, plen=300)]


def many_logit_rows(mk):
    """200 prompts of 2 rows, each finishing: 400 rows of which half feed the LM head."""
    return [mk.prefill(0, 2) for _ in range(200)]


def run_chain(model, runner, items):
    """One step through ``_forward_chain`` on the runner's metadata: the hidden rows it returns."""
    si, rows = runner.prepare(items)
    ids, meta = runner._meta(si)
    with torch.inference_mode():
        h = model._forward_chain(model.embed_tokens(ids), meta, runner.kv_caches)
    return h, meta


def same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    n = a.element_size()
    view = {2: torch.int16, 4: torch.int32}[n]
    return bool(torch.equal(a.contiguous().view(view), b.contiguous().view(view)))
