"""The per-request rules on the logit rows, each with its device tables, its pinned staging and its launch in one place.

`Penalties` (csrc/penalty.hip), `Constraints` (csrc/constrain.hip) and `Guides` (csrc/guide.hip) rewrite the raw rows in front of
everything else.  The runner builds one on the first batch that needs it and then knows two methods:
  * stage(seqs, back, stage_set, base=0): pack what the kernel reads for this batch and queue its copies to the device.  back:
    lookahead entries at the end of token_ids that are not history (the K speculated tokens under verification: the kernel reads those
    from the round's inputs, row by row).  stage_set: which of the two sets of pinned buffers to use (ModelRunner._upload).  base: the
    table slot of the batch's row 0, for the tables that stay on the device from step to step (`take_slots`).
  * apply(lg, rows, rows_per_seq, extras, base=0): adjust `rows` raw logit rows in place.  extras: the extra / extra_ld / extra_n
    keywords of the form the body runs (none: the staged history alone; prefix: row j of a verify also sees inputs 1..j; chain: every
    row also sees the tokens of its draft chain so far).  Rows of sequences without the rule come back untouched.
The host packing of each is a function over numpy arrays (`pack_*`): the classes call it on the views of their pinned buffers, the
CPU tests on plain arrays.  `Logprobs` (csrc/logprob.hip) reads the raw rows before the rules and picks after the token, so it has an
interface of its own, and `PromptLogprobs` (csrc/prompt_logprob.hip) scores the rows of a prefill that no rule ever touches.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from ssd_amd.hip import penalty_ops as HP
from ssd_amd.hip import constrain_ops as HC
from ssd_amd.hip import guide_ops as HG
from ssd_amd.hip import logprob_ops as HL
from ssd_amd.hip import prompt_logprob_ops as HPL

I32_MAX = 2 ** 31 - 1


class RuleSizes(NamedTuple):
    """What a runner tells a rule about itself."""
    seq_cap: int            # sequences a batch can hold: rows of the per-sequence tables
    vocab: int
    K: int                  # speculate_k (0 without speculation): a round shows a row at most K extra tokens
    max_model_len: int
    rows: int               # logit rows one launch can cover
    eos: int                # the engine's EOS when the rule is built; the runner keeps Constraints.eos current
    device: torch.device


class Staging:
    """Pinned mirrors of a list of device tensors, one set per stage set, made on first use: set(stage_set) -> (pinned tensors, their
    numpy views)."""

    def __init__(self, dsts):
        self.dsts = tuple(dsts)
        self._sets: dict = {}

    def set(self, stage_set: int):
        st = self._sets.get(stage_set)
        if st is None:
            pinned = [torch.zeros(d.shape, dtype=d.dtype).pin_memory() for d in self.dsts]
            st = self._sets[stage_set] = (pinned, [t.numpy() for t in pinned])
        return st


def take_slots(owner: list, seq_ids, base: int = 0) -> list[int]:
    """The rows b of a batch whose table slot base + b must receive its sequence's table this step: those whose slot did not hold
    the table of seq_ids[b] (None: the sequence has none and leaves the slot as it is).  owner[slot] is the sequence whose table the
    slot holds; the slots named are theirs from now on.  A large table is a constant of its request, so it travels only when its
    sequence takes a slot it did not have.  A decode, chain or verify batch uses the slots of its rows (base 0); the eager prefill of
    B new requests uses the last B (base = seq_cap - B), which the running batch leaves free while running + new <= max_num_seqs, so
    an arrival does not evict the table of the sequence decoding in row 0."""
    moved = []
    for b, sid in enumerate(seq_ids):
        if sid is not None and owner[base + b] != sid:
            owner[base + b] = sid
            moved.append(b)
    return moved


# ---- penalties and logit bias ------------------------------------------------------------------------------------------------------
def pack_penalties(seqs, back: int, ids, cnt, bias, lens, par) -> None:
    """Every sequence's history table and parameters: unique token ids, (output count << 1) | in prompt, bias -- int32 / int32 / fp32
    [B][L] -- with their length, int32 [B], and fp32 par [3][B] = repetition, presence, frequency.  A sequence without penalties
    reads as off: length 0, parameters 1 / 0 / 0."""
    L = ids.shape[1]
    for b, s in enumerate(seqs):
        if not getattr(s, "has_penalty", False):
            lens[b], par[0, b], par[1, b], par[2, b] = 0, 1.0, 0.0, 0.0
            continue
        tab = s.penalty_table(len(s.token_ids) - back)
        n = len(tab)
        if n > L:
            raise ValueError(f"the history of sequence {s.seq_id} ({n} distinct token and logit_bias ids) does not fit the penalty "
                             f"table of {L} entries (max_model_len + {Penalties.MAX_BIAS})")
        if n:
            vals = np.array(list(tab.values()), dtype=np.float64)
            ids[b, :n] = np.clip(np.fromiter(tab.keys(), dtype=np.int64, count=n), -1, I32_MAX)
            cnt[b, :n] = (vals[:, 0].astype(np.int64) << 1) | vals[:, 1].astype(np.int64)
            bias[b, :n] = vals[:, 2]
        lens[b], par[0, b], par[1, b], par[2, b] = n, s.repetition_penalty, s.presence_penalty, s.frequency_penalty


class Penalties:
    MAX_BIAS = 1024         # logit_bias entries one request may carry: the history table holds max_model_len + this many ids

    def __init__(self, z: RuleSizes):
        assert z.K + 1 <= HP.MAX_EXTRA + 1, "speculate_k exceeds SSD_PENALTY_MAX_EXTRA"
        B, L = z.seq_cap, z.max_model_len + self.MAX_BIAS
        dev = dict(device=z.device)
        self.V, self.tab_ld = z.vocab, L
        self.d_ids = torch.zeros(B, L, dtype=torch.int32, **dev)
        self.d_cnt = torch.zeros(B, L, dtype=torch.int32, **dev)
        self.d_bias = torch.zeros(B, L, dtype=torch.float32, **dev)
        self.d_len = torch.zeros(B, dtype=torch.int32, **dev)
        self.d_par = torch.zeros(3, B, dtype=torch.float32, **dev)
        self._staging = Staging((self.d_ids, self.d_cnt, self.d_bias, self.d_len, self.d_par))

    def stage(self, seqs, back: int, stage_set: int, base: int = 0) -> None:
        """(No table stays on the device: the history grows every step, so base has nothing to select.)"""
        pinned, views = self._staging.set(stage_set)
        pack_penalties(seqs, back, *views)
        B = len(seqs)
        for d, h in zip(self._staging.dsts[:4], pinned):
            d[:B].copy_(h[:B], non_blocking=True)
        self.d_par.copy_(pinned[4], non_blocking=True)

    def apply(self, lg: torch.Tensor, rows: int, rows_per_seq: int, extras: dict, base: int = 0) -> None:
        V, par = self.V, self.d_par
        HP.penalize_rows(lg, V, rows, V, rows_per_seq, self.d_ids, self.d_cnt, self.d_bias, self.tab_ld, self.d_len, par[0], par[1],
                         par[2], **extras)


# ---- min_tokens, allowed ids, bad words --------------------------------------------------------------------------------------------
def pack_constraints(seqs, back: int, V: int, eos: int, owner: list, base: int, bits, tok, off, stop, tail, par):
    """Every sequence's stop list (+ the EOS) held back by min_tokens, flattened bad words with the last tokens the host knows, and
    int32 par [5][B] = allow_on, min_left, stop_len, bw_n, tail_len; a sequence without constraints reads as par[:, b] = 0.  The
    allow mask (uint32 words moved as int32 bits; 16 KB at a 128 K vocabulary) is written to bits[b] only for the rows
    take_slots(owner, ..., base) names.  Returns (those rows, some sequence has bad words)."""
    any_words = False
    for b, s in enumerate(seqs):
        par[:, b] = 0
        if not getattr(s, "has_constraint", False):
            continue
        upto = len(s.token_ids) - back
        if s.allowed_token_ids is not None:
            par[0, b] = 1
        if s.min_tokens > 0:
            stops = s.stop_list(eos)
            if len(stops) > HC.MAX_STOP:
                raise ValueError(f"sequence {s.seq_id} has {len(stops)} stop ids (the EOS included) to hold back under min_tokens: "
                                 f"at most {HC.MAX_STOP}")
            stop[b, :len(stops)] = np.clip(stops, -1, I32_MAX)
            par[1, b], par[2, b] = s.min_left(upto), len(stops)
        if s.bad_words:
            flat, offs = s.bad_words_flat
            tok[b, :len(flat)] = np.clip(flat, -1, I32_MAX)
            off[b, :len(offs)] = offs
            t = s.constraint_tail(HC.TAIL_LD, upto)
            tail[b, :len(t)] = np.clip(t, -1, I32_MAX)
            par[3, b], par[4, b] = len(s.bad_words), len(t)
            any_words = True
    moved = take_slots(owner, [s.seq_id if getattr(s, "allowed_token_ids", None) is not None else None for s in seqs], base)
    for b in moved:
        bits[b] = seqs[b].allow_bits(V).view(np.int32)
    return moved, any_words


class Constraints:
    def __init__(self, z: RuleSizes):
        assert z.K + 1 <= HC.MAX_EXTRA + 1, "speculate_k exceeds SSD_CONSTRAIN_MAX_EXTRA"
        B = z.seq_cap
        dev = dict(device=z.device)
        self.V, self.eos = z.vocab, z.eos
        self.d_bits = torch.zeros(B, HC.mask_words(z.vocab), dtype=torch.int32, **dev)      # one slot per sequence (take_slots)
        self.d_tok = torch.zeros(B, HC.MAX_WORD_TOKENS, dtype=torch.int32, **dev)
        self.d_off = torch.zeros(B, HC.MAX_WORDS + 1, dtype=torch.int32, **dev)
        self.d_stop = torch.zeros(B, HC.MAX_STOP, dtype=torch.int32, **dev)
        self.d_tail = torch.zeros(B, HC.TAIL_LD, dtype=torch.int32, **dev)
        self.d_par = torch.zeros(5, B, dtype=torch.int32, **dev)
        self._staging = Staging((self.d_bits, self.d_tok, self.d_off, self.d_stop, self.d_tail, self.d_par))
        self.owner = [None] * B

    def stage(self, seqs, back: int, stage_set: int, base: int = 0) -> None:
        pinned, views = self._staging.set(stage_set)
        moved, any_words = pack_constraints(seqs, back, self.V, self.eos, self.owner, base, *views)
        B = len(seqs)
        for b in moved:
            self.d_bits[base + b].copy_(pinned[0][b], non_blocking=True)
        for d, h, on in zip(self._staging.dsts[1:5], pinned[1:5], (any_words, any_words, True, any_words)):
            if on:
                d[:B].copy_(h[:B], non_blocking=True)
        self.d_par.copy_(pinned[5], non_blocking=True)

    def apply(self, lg: torch.Tensor, rows: int, rows_per_seq: int, extras: dict, base: int = 0) -> None:
        V, par = self.V, self.d_par         # (the per-step values are indexed by the batch row, the mask by the slot)
        HC.constrain_rows(lg, V, rows, V, rows_per_seq, allow_on=par[0], allow_bits=self.d_bits[base:], min_left=par[1],
                          stop_ids=self.d_stop, stop_len=par[2], bw_tok=self.d_tok, bw_off=self.d_off, bw_n=par[3],
                          tail=self.d_tail, tail_ld=HC.TAIL_LD, tail_len=par[4], **extras)


# ---- token automata ----------------------------------------------------------------------------------------------------------------
def pack_guides(seqs, back: int, owner: list, base: int, par) -> list[int]:
    """int32 par [3][B] = guide_on, the state in front of every sequence's first row (Sequence.guide_state: derived from token_ids;
    the kernel walks the round's own tokens from there) and n_states; a sequence without a guide reads as par[:, b] = 0.  Returns the
    rows whose automaton must travel (take_slots)."""
    for b, s in enumerate(seqs):
        par[:, b] = 0
        a = getattr(s, "guide", None)
        if a is not None:
            par[0, b], par[1, b], par[2, b] = 1, s.guide_state(len(s.token_ids) - back), a.num_states
    return take_slots(owner, [s.seq_id if getattr(s, "guide", None) is not None else None for s in seqs], base)


class Guides:
    def __init__(self, z: RuleSizes):
        assert z.K + 1 <= HG.MAX_EXTRA + 1, "speculate_k exceeds SSD_GUIDE_MAX_EXTRA"
        B, S, E = z.seq_cap, HG.MAX_STATES, HG.MAX_EDGES
        dev = dict(device=z.device)
        self.V = z.vocab
        # one automaton slot per sequence at the strides of the largest automaton a request may carry (2.2 MB a slot)
        self.d_off = torch.zeros(B, S + 1, dtype=torch.int32, **dev)         # CSR offsets
        self.d_dflt = torch.full((B, S), -1, dtype=torch.int32, **dev)
        self.d_tok = torch.zeros(B, E, dtype=torch.int32, **dev)
        self.d_next = torch.zeros(B, E, dtype=torch.int32, **dev)
        self.d_par = torch.zeros(3, B, dtype=torch.int32, **dev)
        self.d_state = torch.full((max(z.rows, B),), -1, dtype=torch.int32, **dev)     # the state in front of every logit row
        self._staging = Staging((self.d_par,))
        self.owner = [None] * B

    def stage(self, seqs, back: int, stage_set: int, base: int = 0) -> None:
        """The used part of a table travels from the pinned copy its sequence keeps (Sequence.guide_pinned: made once per request;
        the automaton is immutable, so it is never rewritten under a copy in flight)."""
        (pinned,), (par,) = self._staging.set(stage_set)
        for b in pack_guides(seqs, back, self.owner, base, par):
            a, flat, at = seqs[b].guide, seqs[b].guide_pinned(), 0
            n, m = a.num_states, a.num_edges
            for d, k in ((self.d_off, n + 1), (self.d_dflt, n), (self.d_tok, m), (self.d_next, m)):
                if k:
                    d[base + b, :k].copy_(flat[at:at + k], non_blocking=True)
                at += k
        self.d_par.copy_(pinned, non_blocking=True)

    def apply(self, lg: torch.Tensor, rows: int, rows_per_seq: int, extras: dict, base: int = 0) -> None:
        """The walk from the staged states through the tokens each row sees, then the rows kernel."""
        V, par, o = self.V, self.d_par, base        # (the per-step values are indexed by the batch row, the tables by the slot)
        tables = (par[2], self.d_off[o:], self.d_dflt[o:], self.d_tok[o:], self.d_next[o:], HG.MAX_STATES, HG.MAX_EDGES)
        HG.guide_walk(self.d_state, rows, rows_per_seq, par[0], par[1], *tables, **extras)
        HG.guide_rows(lg, V, rows, V, self.d_state, rows_per_seq, *tables)


RULES = (("pen", Penalties), ("con", Constraints), ("gd", Guides))      # Sampling field -> rule, in the order they run


# ---- log-probabilities -------------------------------------------------------------------------------------------------------------
class Logprobs:
    """Raw log-probabilities of the target's rows: `rows` runs behind compute_logits and in front of the rules, `pick` /
    `pick_verify` behind the token, `post` queues the copies the host reads and `records` turns them into the request's records."""

    def __init__(self, z: RuleSizes):
        R, V = z.rows, z.vocab
        dev = dict(device=z.device)
        self.V = V
        self.d_ntop = torch.full((z.seq_cap,), -1, dtype=torch.int32, **dev)
        self.d_lse = torch.zeros(R, dtype=torch.float32, **dev)
        self.d_out = torch.zeros(R, dtype=torch.float32, **dev)
        self.d_top_val = torch.zeros(R, HL.MAX_N, dtype=torch.float32, **dev)
        self.d_top_id = torch.zeros(R, HL.MAX_N, dtype=torch.int32, **dev)
        self.d_ws = torch.zeros(HL.logprob_rows_ws_bytes(R, V) // 4, dtype=torch.float32, **dev)
        self.d_raw = None       # rows x V bf16: the copy of the raw rows a penalised batch picks from (on ITS first use)
        self.h_out = torch.zeros(R, dtype=torch.float32).pin_memory()
        self.h_top_val = torch.zeros(R, HL.MAX_N, dtype=torch.float32).pin_memory()
        self.h_top_id = torch.zeros(R, HL.MAX_N, dtype=torch.int32).pin_memory()
        self._staging = Staging((self.d_ntop,))

    def stage(self, seqs, stage_set: int, pen: bool) -> None:
        """The N of every sequence; -1 = did not ask: the kernels skip its rows.  pen: the batch is penalised."""
        if pen and self.d_raw is None:
            self.d_raw = torch.zeros(self.d_lse.shape[0], self.V, dtype=torch.bfloat16, device=self.d_lse.device)
        (pinned,), (ntop,) = self._staging.set(stage_set)
        B = len(seqs)
        ntop[:B] = [-1 if getattr(s, "logprobs", None) is None else int(s.logprobs) for s in seqs]
        self.d_ntop[:B].copy_(pinned[:B], non_blocking=True)

    def rows(self, logits: torch.Tensor, rows: int, rows_per_param: int, pen: bool) -> None:
        """Log-sum-exp and top entries of the RAW rows.  A penalised batch also keeps a copy of them (penalties rewrite entries a
        chosen token may sit on; truncation and bans only write -inf over entries that can no longer be chosen, so the live rows
        serve there)."""
        V = self.V
        HL.logprob_rows(logits, V, rows, V, self.d_ntop, rows_per_param, self.d_lse, self.d_top_val, self.d_top_id, self.d_ws,
                        raw_copy=self.d_raw if pen else None, raw_ld=V if pen else 0)

    def pick(self, logits: torch.Tensor, rows: int, tokens: torch.Tensor, pen: bool) -> None:
        """d_out = raw log-probability of `tokens`, row by row (decode and prefill rows: one sequence each)."""
        V = self.V
        HL.logprob_pick(self.d_raw if pen else logits, V, rows, V, tokens, self.d_lse, self.d_ntop, 1, self.d_out)

    def pick_verify(self, logits: torch.Tensor, B: int, K: int, ids, accept, recovery, pen: bool) -> None:
        """The same for the accepted inputs and the recovery token of every sequence of a verify."""
        V = self.V
        HL.logprob_pick_verify(self.d_raw if pen else logits, V, B, K, V, ids, accept, recovery, self.d_lse, self.d_ntop, self.d_out)

    def post(self, rows: int) -> None:
        """Queue the D2H copies of what the host reads, in front of the synchronise the step performs anyway (lse stays on the device)."""
        self.h_out[:rows].copy_(self.d_out[:rows], non_blocking=True)
        self.h_top_val[:rows].copy_(self.d_top_val[:rows], non_blocking=True)
        self.h_top_id[:rows].copy_(self.d_top_id[:rows], non_blocking=True)

    def records(self, seqs, row_tokens, single: bool = False):
        """The records of `seqs` from the pinned mirrors (after the synchronise).  row_tokens: per sequence the (row, token) pairs of
        its tokens, in order; sequences that did not ask get None.  single: one record per sequence instead of a list."""
        n = 1 + max(r for pairs in row_tokens for r, _ in pairs)
        lp, tv, ti = self.h_out[:n].tolist(), self.h_top_val[:n].tolist(), self.h_top_id[:n].tolist()
        out = []
        for s, pairs in zip(seqs, row_tokens):
            N = getattr(s, "logprobs", None)
            if N is None:
                out.append(None)
                continue
            recs = []
            for r, tok in pairs:
                k = sum(1 for i in ti[r][:N] if i >= 0)         # min(N, V): slots past the row's entries hold -1 / -inf
                recs.append({"token_id": int(tok), "logprob": lp[r], "top_ids": ti[r][:k], "top_logprobs": tv[r][:k]})
            out.append(recs[0] if single else recs)
        return out


class PromptLogprobs:
    """Raw log-probabilities and ranks of the prompt tokens of a prefill (SamplingParams.prompt_logprobs): `stage` uploads the N of
    every ROW, `chunk` scores one chunk of rows from its logits, `post` queues the copies the host reads and `records` turns them into
    the requests' lists.  Row t of a prefill holds the distribution that predicts the token of row t + 1, so the token array is the
    prefill's own id array one row on; the last row of every sequence predicts the generated token (logprobs= covers it) and is
    skipped, as is every row of a sequence that does not ask."""

    def __init__(self, z: RuleSizes, max_rows: int):
        R = max_rows            # max_num_batched_tokens: the rows one prefill can have
        dev = dict(device=z.device)
        self.V = z.vocab
        self.d_ntop = torch.full((R,), -1, dtype=torch.int32, **dev)
        self.d_rows = torch.arange(R, dtype=torch.int32, **dev)       # the consecutive row indices a chunk's norm gathers
        self.d_lse = torch.zeros(R, dtype=torch.float32, **dev)
        self.d_out = torch.zeros(R, dtype=torch.float32, **dev)
        self.d_rank = torch.zeros(R, dtype=torch.int32, **dev)
        self.d_top_val = torch.zeros(R, HL.MAX_N, dtype=torch.float32, **dev)
        self.d_top_id = torch.zeros(R, HL.MAX_N, dtype=torch.int32, **dev)
        self.h_out = torch.zeros(R, dtype=torch.float32).pin_memory()
        self.h_rank = torch.zeros(R, dtype=torch.int32).pin_memory()
        self.h_top_val = torch.zeros(R, HL.MAX_N, dtype=torch.float32).pin_memory()
        self.h_top_id = torch.zeros(R, HL.MAX_N, dtype=torch.int32).pin_memory()
        self._staging = Staging((self.d_ntop,))
        self.chunk_rows = 0     # the chunk buffers exist for this many rows (made on first use, remade when the runner's size changes)
        self.d_logits = self.d_frag = self.d_ws = None

    @staticmethod
    def row_counts(seqs, starts) -> list[int]:
        """n_top of every row of a prefill whose sequence b owns rows starts[b] .. starts[b + 1]: the sequence's N, -1 at its last
        row and at every row of a sequence that does not need its prompt scored."""
        ntop = []
        for b, s in enumerate(seqs):
            n = starts[b + 1] - starts[b]
            ask = getattr(s, "needs_prompt_logprobs", False)
            ntop.extend([int(s.prompt_logprobs) if ask else -1] * (n - 1) + [-1])
        return ntop

    def stage(self, ntop: list[int], stage_set: int) -> None:
        (pinned,), (view,) = self._staging.set(stage_set)
        T = len(ntop)
        view[:T] = ntop
        self.d_ntop[:T].copy_(pinned[:T], non_blocking=True)

    def buffers(self, chunk_rows: int, h: int, frag_numel: int):
        """(norm output fragment, logits) of a chunk of up to chunk_rows rows."""
        if self.chunk_rows != chunk_rows:
            dev = dict(device=self.d_lse.device)
            self.d_logits = torch.zeros(chunk_rows, self.V, dtype=torch.bfloat16, **dev)
            self.d_frag = torch.zeros(frag_numel, dtype=torch.bfloat16, **dev)
            self.d_ws = torch.zeros(HPL.logprob_known_ws_bytes(chunk_rows, self.V) // 4, dtype=torch.float32, **dev)
            self.chunk_rows = chunk_rows
        return self.d_frag, self.d_logits

    def chunk(self, r0: int, n: int, ids: torch.Tensor) -> None:
        """Score rows r0 .. r0 + n of the prefill from the chunk's logits; ids: the prefill's int64 id array."""
        V = self.V
        HPL.logprob_rows_known(self.d_logits, V, n, V, self.d_ntop[r0:], ids[r0 + 1:], self.d_lse[r0:], self.d_top_val[r0:],
                               self.d_top_id[r0:], self.d_out[r0:], self.d_rank[r0:], self.d_ws)

    def post(self, rows: int) -> None:
        """Queue the D2H copies of what the host reads, in front of the synchronise the prefill performs anyway."""
        for h, d in ((self.h_out, self.d_out), (self.h_rank, self.d_rank), (self.h_top_val, self.d_top_val), (self.h_top_id, self.d_top_id)):
            h[:rows].copy_(d[:rows], non_blocking=True)

    def records(self, seqs, starts, scored: bool = True):
        """Per sequence that needs them the list for its prompt -- None, then one record per further prompt token -- from the pinned
        mirrors (after the synchronise); None for the others.  scored = False: no row was scored (one-token prompts only)."""
        T = starts[-1]
        if scored:
            lp, rk, tv, ti = self.h_out[:T].tolist(), self.h_rank[:T].tolist(), self.h_top_val[:T].tolist(), self.h_top_id[:T].tolist()
        out = []
        for b, s in enumerate(seqs):
            if not getattr(s, "needs_prompt_logprobs", False):
                out.append(None)
                continue
            N, recs = s.prompt_logprobs, [None]
            for i in range(1, starts[b + 1] - starts[b]):
                r = starts[b] + i - 1
                k = sum(1 for j in ti[r][:N] if j >= 0)
                recs.append({"token_id": int(s[i]), "logprob": lp[r], "rank": rk[r], "top_ids": ti[r][:k], "top_logprobs": tv[r][:k]})
            out.append(recs)
        return out
