"""Per-request state.  Field names and meanings follow the reference (ssd/engine/sequence.py:14-120) because the
scheduler / speculator / verifier contract is expressed in them: ``num_cached_tokens`` and
``num_draft_cached_tokens`` count KV positions valid in the target / draft cache, ``recovery_token_id`` is the
token sampled by the last verify (or prefill) that is NOT yet in ``token_ids``, and
``last_spec_step_accepted_len`` (-1 before the first step) feeds the async speculation-cache key."""
from __future__ import annotations

from enum import Enum, auto
from itertools import count

import numpy as np

from ssd_amd.sampling_params import SamplingParams


class SequenceStatus(Enum):
    WAITING = auto()
    RUNNING = auto()
    FINISHED = auto()


class Sequence:
    counter = count()       # process-global, monotonically increasing seq ids (reference sequence.py:15,28)
    block_size = 256        # set by the engine from Config.kvcache_block_size

    def __init__(self, token_ids: list[int], sampling_params: SamplingParams | None = None, guide=None, lora=None):
        """guide: the TokenAutomaton LLMEngine.add_request compiled from guided_choice_ids (it needs the engine's EOS).
        lora: (slot, identity) of the adapter registration LLMEngine.add_request resolved SamplingParams.lora to."""
        sp = sampling_params or SamplingParams()
        # LoRA adapter (ssd_amd/lora.py; None / -1 = off): the name, the slot the target's rows name, and the 64-bit identity of the
        # registration the target's block hashes start from.  They stay with the sequence through preemption and re-prefill
        self.lora = sp.lora if lora is not None else None
        self.lora_slot, self.lora_id = lora if lora is not None else (-1, -1)
        self.seq_id = next(Sequence.counter)
        self.status = SequenceStatus.WAITING
        self.token_ids = list(token_ids)
        self.last_token = self.token_ids[-1]
        self.num_tokens = len(self.token_ids)
        self.num_prompt_tokens = self.num_tokens
        self.num_cached_tokens = 0
        self.num_draft_cached_tokens = 0
        self.block_table: list[int] = []
        self.draft_block_table: list[int] = []
        self.last_spec_step_accepted_len = -1
        self.recovery_token_id: int | None = None
        # the prefill's token once LLMEngine.generate handed it to the stream ahead of the first speculation round; consumed
        # (cleared) by the append that puts it into the sequence -- a LATER preemption must not resurrect it
        self.first_token_streamed: int | None = None
        self.temperature = sp.temperature
        self.draft_temperature = sp.draft_temperature
        self.top_k, self.top_p, self.min_p = sp.top_k, sp.top_p, sp.min_p       # logit filter (0 / 1.0 / 0.0 = off)
        # penalties and logit bias (include/ssd_hip_penalty.h; 1.0 / 0.0 / 0.0 / None = off)
        self.repetition_penalty, self.presence_penalty = float(sp.repetition_penalty), float(sp.presence_penalty)
        self.frequency_penalty = float(sp.frequency_penalty)
        self.logit_bias = {int(t): float(v) for t, v in sp.logit_bias.items()} if sp.logit_bias else None
        # the sparse history behind them: token id -> [output count, in prompt, bias], kept for token_ids[:_pen_n].  "Prompt" is the
        # request's own prompt for good: a preemption turns completions into prompt for the scheduler, not for the penalties
        self.num_request_prompt_tokens = self.num_tokens
        self._pen: dict[int, list] | None = None
        self._pen_n = 0
        if self.has_penalty:
            self._pen = {t: [0, False, v] for t, v in (self.logit_bias or {}).items()}
        self.max_new_tokens = sp.max_new_tokens
        self.ignore_eos = sp.ignore_eos
        # log-probabilities (include/ssd_hip_logprob.h): the N asked for (None = off) and one record {"token_id", "logprob", "top_ids",
        # "top_logprobs"} per generated token -- record i belongs to token_ids[num_request_prompt_tokens + i]: like the penalties'
        # history it is keyed from the request's own prompt, because a preemption moves num_prompt_tokens.  recovery_logprob is the
        # record of recovery_token_id; it joins the list in the round that commits that token
        self.logprobs = sp.logprobs
        self.logprob_records: list[dict] = []
        self.recovery_logprob: dict | None = None
        # prompt log-probabilities (include/ssd_hip_prompt_logprob.h): the N asked for (None = off) and, once the first prefill has
        # scored the request's own prompt, one entry per prompt token -- None for token 0, then {"token_id", "logprob", "rank",
        # "top_ids", "top_logprobs"}.  Stored once: the re-prefill after a preemption finds them and does not ask again
        self.prompt_logprobs = sp.prompt_logprobs
        self.prompt_logprob_records: list | None = None
        # per-request seed (include/ssd_hip_seed.h; None = the engine's stream).  The stream is keyed by absolute positions, so a
        # preempted sequence's recomputed prefill draws the numbers the position always had
        self.seed = sp.seed
        # hard constraints (include/ssd_hip_constrain.h; None / 0 = off) and stop ids.  What the runner uploads is kept here: the stop
        # list and the flattened bad words for good, the allow bitmask once its width is known (allow_bits); the tail and the output
        # count are functions of token_ids and are derived, not mirrored, so a rollback or a preemption cannot leave them behind.
        # "Output" counts from the request's own prompt, like the penalties' history
        self.stop_token_ids = tuple(dict.fromkeys(int(t) for t in sp.stop_token_ids)) if sp.stop_token_ids else ()
        self.stop_reason: int | None = None         # the stop id that ended the request (the scheduler writes it)
        self.min_tokens = sp.min_tokens
        self.allowed_token_ids = sorted({int(t) for t in sp.allowed_token_ids}) if sp.allowed_token_ids is not None else None
        self.bad_words = tuple(dict.fromkeys(tuple(int(t) for t in w) for w in sp.bad_words_ids)) if sp.bad_words_ids else ()
        self.bad_words_flat = ([t for w in self.bad_words for t in w],
                               [sum(len(w) for w in self.bad_words[:i]) for i in range(len(self.bad_words) + 1)])
        self._allow_bits = None
        # guided decoding (ssd_amd/guide.py, include/ssd_hip_guide.h; None = off): the automaton, and its state after every output
        # position walked so far -- _guide_states[i] is the state after i output tokens.  Like the tail above the state is a function
        # of token_ids: guide_state derives it on demand and restore cuts it back with the tokens
        self.guide = guide if guide is not None else sp.guided_automaton
        self._guide_states = [self.guide.start] if self.guide is not None else None
        self._guide_pinned = None
        # EAGLE-3 (reference sequence.py:23-24,47-51): the target activation that conditions the next recovery token, and
        # the accepted draft tokens + their target activations that the draft re-deposits ("extends") at the next glue
        self.last_target_hidden_state = None
        self.extend_eagle_acts = None
        self.extend_token_ids: list[int] | None = None
        self.extend_count = 0

    def __len__(self) -> int:
        return self.num_tokens

    def __getitem__(self, key):
        return self.token_ids[key]

    @property
    def has_filter(self) -> bool:
        return self.top_k > 0 or self.top_p < 1.0 or self.min_p > 0.0

    @property
    def has_penalty(self) -> bool:
        return (self.repetition_penalty != 1.0 or self.presence_penalty != 0.0 or self.frequency_penalty != 0.0
                or bool(self.logit_bias))

    @property
    def needs_prompt_logprobs(self) -> bool:
        """The next prefill must score the prompt: the request asked and has no records yet.  While this holds the target's block
        manager gives the sequence no prefix hit (BlockManager.allocate), so every row to be scored is computed."""
        return self.prompt_logprobs is not None and self.prompt_logprob_records is None

    def store_prompt_logprobs(self, records: list) -> None:
        assert self.needs_prompt_logprobs and len(records) == self.num_request_prompt_tokens
        self.prompt_logprob_records = records

    @property
    def has_constraint(self) -> bool:
        """Something the constraint kernel enforces is on (stop_token_ids alone is host work)."""
        return self.min_tokens > 0 or self.allowed_token_ids is not None or bool(self.bad_words)

    def allow_bits(self, V: int) -> np.ndarray:
        """uint32 [ceil(V / 32)]: bit t & 31 of word t >> 5 is set for every allowed id below V.  Built once per request."""
        assert self.allowed_token_ids is not None
        if self._allow_bits is None or self._allow_bits[0] != V:
            ids = np.array([t for t in self.allowed_token_ids if t < V], dtype=np.int64)
            bits = np.zeros((V + 31) // 32, dtype=np.uint32)
            np.bitwise_or.at(bits, ids >> 5, np.left_shift(np.uint32(1), (ids & 31).astype(np.uint32)))
            self._allow_bits = (V, bits)
        return self._allow_bits[1]

    def stop_list(self, eos: int) -> list[int]:
        """What min_tokens keeps from being generated: the stop ids and, unless the sequence ignores it, the EOS."""
        return list(dict.fromkeys(list(self.stop_token_ids) + ([] if self.ignore_eos else [int(eos)])))

    def num_output_tokens(self, upto: int | None = None) -> int:
        """Tokens of token_ids[:upto] behind the request's own prompt."""
        return max(0, (len(self.token_ids) if upto is None else upto) - self.num_request_prompt_tokens)

    def min_left(self, upto: int | None = None) -> int:
        """Output tokens still missing to min_tokens in front of the row that predicts token_ids[upto]."""
        return max(0, self.min_tokens - self.num_output_tokens(upto))

    def constraint_tail(self, n: int, upto: int | None = None) -> list[int]:
        """The last n tokens of token_ids[:upto]: what a bad word's prefix is matched against."""
        upto = len(self.token_ids) if upto is None else upto
        return self.token_ids[max(0, upto - n):upto]

    def stops_at(self, token: int, index: int, eos: int) -> bool:
        """token, sitting at token_ids[index], ends the request: the EOS (unless ignored) or a stop id, and not before min_tokens
        output tokens stand in front of it."""
        if index - self.num_request_prompt_tokens < self.min_tokens:
            return False
        return (not self.ignore_eos and token == eos) or token in self.stop_token_ids

    def guide_state(self, upto: int | None = None) -> int:
        """The automaton's state after the output tokens of token_ids[:upto] (counted from the request's own prompt): the state in
        front of the row that predicts token_ids[upto].  -1: a token was not allowed where it stands, nothing guides from there on.
        Kept incrementally, one state per output position; only what lies in front of `upto` is ever walked, so the placeholders
        of a lookahead (negative ids, always behind `upto`) are not."""
        assert self.guide is not None, "guide_state() of a sequence without a guide"
        st, ids, P = self._guide_states, self.token_ids, self.num_request_prompt_tokens
        n = max(0, (len(ids) if upto is None else upto) - P)
        assert P + n <= len(ids)
        while len(st) <= n:
            t = ids[P + len(st) - 1]
            st.append(self.guide.delta(st[-1], t) if t >= 0 else -1)
        return st[n]

    def guide_pinned(self):
        """The automaton's flattened tables -- edge_off, dflt, edge_tok, edge_next, one behind the other -- as one pinned int32 tensor:
        what the runners upload from when the sequence takes a table slot.  Made once per request and shared by the target and the
        draft runner."""
        if self._guide_pinned is None:
            import torch
            a = self.guide
            self._guide_pinned = torch.from_numpy(np.concatenate([a.edge_off, a.dflt, a.edge_tok, a.edge_next])).pin_memory()
        return self._guide_pinned

    def penalty_table(self, upto: int | None = None) -> dict[int, list]:
        """token id -> [occurrences after the request's prompt, occurs in the prompt, bias] over token_ids[:upto] (default: all of
        them) plus the biased ids; placeholders (negative ids) are not history.  Kept incrementally: a call accounts for the tokens
        appended since the last one and takes back those beyond `upto`; `restore` takes back what it cuts off.  Only sequences with
        has_penalty keep one."""
        assert self._pen is not None, "penalty_table() of a sequence without penalties"
        self._pen_sync(len(self.token_ids) if upto is None else upto)
        return self._pen

    def _pen_sync(self, upto: int) -> None:
        pen, ids, P = self._pen, self.token_ids, self.num_request_prompt_tokens
        assert 0 <= upto <= len(ids)
        if upto < self._pen_n and upto < P:         # cutting into the prompt: another occurrence may remain, recount
            self._pen = pen = {t: [0, False, v] for t, v in (self.logit_bias or {}).items()}
            self._pen_n = 0
        for i in range(self._pen_n, upto):
            t = ids[i]
            if t < 0:
                continue
            e = pen.get(t)
            if e is None:
                e = pen[t] = [0, False, 0.0]
            if i < P:
                e[1] = True
            else:
                e[0] += 1
        for i in range(upto, self._pen_n):
            t = ids[i]
            if t < 0:
                continue
            e = pen[t]
            e[0] -= 1
            if e[0] == 0 and not e[1] and not (self.logit_bias and t in self.logit_bias):
                del pen[t]
        self._pen_n = upto

    @property
    def is_finished(self) -> bool:
        return self.status is SequenceStatus.FINISHED

    @property
    def num_completion_tokens(self) -> int:
        return self.num_tokens - self.num_prompt_tokens

    @property
    def prompt_token_ids(self) -> list[int]:
        return self.token_ids[:self.num_prompt_tokens]

    @property
    def completion_token_ids(self) -> list[int]:
        return self.token_ids[self.num_prompt_tokens:]

    @property
    def completion_logprobs(self) -> list[dict]:
        """The records of completion_token_ids (after a preemption: of the tokens generated since, as completion_token_ids)."""
        return self.logprob_records[self.num_prompt_tokens - self.num_request_prompt_tokens:]

    @property
    def num_blocks(self) -> int:
        return -(-self.num_tokens // self.block_size)

    @property
    def num_cached_blocks(self) -> int:
        return -(-self.num_cached_tokens // self.block_size)

    @property
    def num_draft_cached_blocks(self) -> int:
        return -(-self.num_draft_cached_tokens // self.block_size)

    @property
    def last_block_num_tokens(self) -> int:
        return self.num_tokens - (self.num_cached_blocks - 1) * self.block_size

    @property
    def last_block_num_tokens_draft(self) -> int:
        return self.num_tokens - (self.num_draft_cached_blocks - 1) * self.block_size

    def block(self, i: int) -> list[int]:
        assert 0 <= i < self.num_blocks
        return self.token_ids[i * self.block_size:(i + 1) * self.block_size]

    def append_token(self, token_id: int) -> None:
        self.token_ids.append(token_id)
        self.last_token = token_id
        self.num_tokens += 1
        self.first_token_streamed = None

    # -- speculation bookkeeping: the (K+1)-token lookahead is applied and rolled back around one
    #    speculate+verify round exactly as SpecDecodeStep.decode does (ssd/engine/step.py:97-145) --
    def snapshot(self):
        return (len(self.token_ids), self.num_tokens, self.last_token, self.num_draft_cached_tokens, self.num_cached_tokens)

    def restore(self, snap) -> None:
        n, self.num_tokens, self.last_token, self.num_draft_cached_tokens, self.num_cached_tokens = snap
        if self._pen is not None and self._pen_n > n:       # the history forgets the lookahead tokens before they go
            self._pen_sync(n)
        if self._guide_states is not None:                  # ... and so do the guide's states
            del self._guide_states[max(1, n - self.num_request_prompt_tokens + 1):]
        del self.token_ids[n:]
