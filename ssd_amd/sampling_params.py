"""SamplingParams -- the reference's fields and defaults (ssd/sampling_params.py:4-9) plus the truncation every other LLM.generate offers:
top_k / top_p / min_p, applied in the Hugging Face order after the temperature (include/ssd_hip_filter.h has the exact semantics), and,
before the temperature, repetition / presence / frequency penalties and logit bias (include/ssd_hip_penalty.h).

``logprobs=N`` asks for the log-probability of every generated token (N = 0) and, beside it, for the N most probable tokens of that
position (N = 1..20).  They are RAW log-probabilities: log_softmax of the target's bf16 logits, taken before penalties, logit bias,
temperature and truncation (include/ssd_hip_logprob.h) -- whatever the decoding mode, the target's distribution.

``prompt_logprobs=N`` asks the same of the request's own prompt: for every prompt token but the first its raw log-probability under the
target's distribution at the position in front of it, its rank there (1 = the most probable token; ties count against it, as in vLLM)
and, for N = 1..20, the N most probable tokens of that position (include/ssd_hip_prompt_logprob.h).  The request's output gains the key
``"prompt_logprobs"``: a list as long as the prompt whose element 0 is None.  The prompt is then scored in the prefill that computes
it, so the request takes no prefix-cache hit (later requests still hit the blocks it leaves).

``seed=S`` makes a sampled request reproducible: every random number it consumes comes from a stream keyed by (S, absolute token
position, purpose, vocabulary index) (include/ssd_hip_seed.h) instead of the engine's own, which depends on what was sampled before and
on the batch slot.  It has no effect at temperature 0.

Hard constraints (include/ssd_hip_constrain.h): ``allowed_token_ids`` restricts generation to a set of ids, ``bad_words_ids`` bans token
sequences by the Hugging Face NoBadWordsLogitsProcessor rule over prompt + output (a one-token word is always banned; the last token of
a longer word is banned wherever the tokens in front end with the rest of it), ``min_tokens`` keeps the EOS (unless ``ignore_eos``) and
every stop id from being generated while the request has fewer output tokens.  Banned entries become -inf in front of the temperature,
the truncation and the draw; raw log-probabilities are read in front of that.  ``stop_token_ids`` ends the request when one of them is
emitted (the token stays in ``token_ids``, as the EOS does; they apply even with ``ignore_eos``, which concerns the EOS only) and adds
the key ``"stop_reason"`` to the request's output: the stop id that ended it, or None.  Multi-token bad words can leave a position
without any allowed token (every member of a small ``allowed_token_ids`` set banned at once): that is the caller's error and is not
guarded.  ``stop`` strings are not offered: they need a tokenizer.

Guided decoding (ssd_amd/guide.py, include/ssd_hip_guide.h): ``guided_automaton`` is a ``TokenAutomaton``, a deterministic automaton
over token ids; at every position only the tokens its current state allows can be generated, and the state follows the output tokens
from the automaton's start state.  ``guided_choice_ids`` is the common special case: the output is exactly one of the given token
sequences followed by the EOS (``LLMEngine.add_request`` builds the trie with ``TokenAutomaton.from_choices`` and the engine's EOS, so
it cannot go with ``ignore_eos``).  At most one of the two may be given.  The guide bans like the constraints above -- -inf in front of
the temperature, the truncation, the draw and the argmax, raw log-probabilities read in front of it -- and independently of them; a
position at which the composition leaves nothing allowed (``min_tokens`` holding the EOS back at the end of a choice, say) is the
caller's error and is not guarded.  A guided request ends as every request does: on the EOS, a stop id or ``max_new_tokens``.
Compilers from regular expressions or JSON schemas to an automaton need a tokenizer and are not offered.

``lora=name`` runs the request on the target with the adapter registered under that name (``LLM.add_lora``; ssd_amd/lora.py,
include/ssd_hip_lora.h).  The engine needs ``enable_lora=True``; an unknown name is refused by ``LLMEngine.add_request``.  Drafts are
never adapted: the output is exactly the adapted target's, whatever the draft proposes."""
import math
from dataclasses import dataclass

from ssd_amd.guide import TokenAutomaton, check_choices


MAX_LOGPROBS = 20       # SSD_LOGPROB_MAX_N
MAX_STOP_TOKEN_IDS = 64         # SSD_CONSTRAIN_MAX_STOP (under min_tokens the EOS counts too: LLMEngine.add_request knows it)
MAX_BAD_WORDS = 128             # SSD_CONSTRAIN_MAX_WORDS
MAX_BAD_WORD_TOKENS = 1024      # SSD_CONSTRAIN_MAX_WORD_TOKENS
MAX_BAD_WORD_LEN = 16           # SSD_CONSTRAIN_MAX_WORD_LEN


def _is_real(v) -> bool:
    return isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)


def _is_id(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool) and v >= 0


@dataclass
class SamplingParams:
    temperature: float = 1.0
    draft_temperature: float | None = None
    max_new_tokens: int = 256
    ignore_eos: bool = False
    top_k: int = 0              # keep the k most probable tokens (ties at the k-th kept); 0 = off
    top_p: float = 1.0          # keep the smallest set of most probable tokens whose mass reaches top_p; 1.0 = off
    min_p: float = 0.0          # keep tokens whose probability is at least min_p times the largest; 0.0 = off
    repetition_penalty: float = 1.0     # logits of tokens in the prompt or the output: divided by it if >= 0, multiplied if < 0; 1.0 = off
    presence_penalty: float = 0.0       # subtracted once from the logit of every token already in the output; 0.0 = off
    frequency_penalty: float = 0.0      # subtracted per occurrence in the output; 0.0 = off
    logit_bias: dict | None = None      # token id -> value in [-100, 100] added to that token's logit; None = off
    logprobs: int | None = None         # None = off; 0 = each generated token's raw log-probability; 1..20 = also the N most probable
    prompt_logprobs: int | None = None  # None = off; 0 = each prompt token's raw log-probability and rank; 1..20 = also the N most probable
    seed: int | None = None             # None = off (the engine's stream); 0 <= seed < 2**63: the request draws from its own stream
    stop_token_ids: list | None = None      # generation ends when one of these ids is emitted (it stays in token_ids); None = off
    min_tokens: int = 0                     # the EOS and the stop ids cannot be generated before this many output tokens; 0 = off
    allowed_token_ids: list | None = None   # only these ids may be generated; None = off
    bad_words_ids: list | None = None       # token sequences that must not appear (Hugging Face NoBadWordsLogitsProcessor); None = off
    guided_automaton: TokenAutomaton | None = None      # only what the automaton's current state allows may be generated; None = off
    guided_choice_ids: list | None = None   # the output is one of these token sequences, then the EOS; None = off
    lora: str | None = None                 # name of a registered adapter the target applies to this request; None = off

    def __post_init__(self):
        if isinstance(self.top_k, bool) or not isinstance(self.top_k, int) or self.top_k < 0:
            raise ValueError(f"top_k must be an integer >= 0 (0 = off), got {self.top_k!r}")
        if not (0.0 < self.top_p <= 1.0):
            raise ValueError(f"top_p must be in (0, 1] (1 = off), got {self.top_p!r}")
        if not (0.0 <= self.min_p <= 1.0):
            raise ValueError(f"min_p must be in [0, 1] (0 = off), got {self.min_p!r}")
        if not _is_real(self.repetition_penalty) or not self.repetition_penalty > 0.0:
            raise ValueError(f"repetition_penalty must be finite and > 0 (1 = off), got {self.repetition_penalty!r}")
        if not _is_real(self.presence_penalty):
            raise ValueError(f"presence_penalty must be finite (0 = off), got {self.presence_penalty!r}")
        if not _is_real(self.frequency_penalty):
            raise ValueError(f"frequency_penalty must be finite (0 = off), got {self.frequency_penalty!r}")
        if self.logit_bias is not None:
            if not isinstance(self.logit_bias, dict):
                raise ValueError(f"logit_bias must be a dict of token id -> bias or None, got {self.logit_bias!r}")
            for t, v in self.logit_bias.items():
                if isinstance(t, bool) or not isinstance(t, int) or t < 0:
                    raise ValueError(f"logit_bias keys must be integers >= 0, got {t!r}")
                if not _is_real(v) or not -100.0 <= v <= 100.0:
                    raise ValueError(f"logit_bias values must be finite and within [-100, 100], got {v!r} for token {t}")

        if self.logprobs is not None and (isinstance(self.logprobs, bool) or not isinstance(self.logprobs, int)
                                          or not 0 <= self.logprobs <= MAX_LOGPROBS):
            raise ValueError(f"logprobs must be None (off) or an integer in [0, {MAX_LOGPROBS}], got {self.logprobs!r}")
        if self.prompt_logprobs is not None and (isinstance(self.prompt_logprobs, bool) or not isinstance(self.prompt_logprobs, int)
                                                 or not 0 <= self.prompt_logprobs <= MAX_LOGPROBS):
            raise ValueError(f"prompt_logprobs must be None (off) or an integer in [0, {MAX_LOGPROBS}], got {self.prompt_logprobs!r}")
        if self.seed is not None and (isinstance(self.seed, bool) or not isinstance(self.seed, int) or not 0 <= self.seed < 2 ** 63):
            raise ValueError(f"seed must be None (off) or an integer in [0, 2**63), got {self.seed!r}")
        if self.stop_token_ids is not None:
            if not isinstance(self.stop_token_ids, (list, tuple)) or not all(_is_id(t) for t in self.stop_token_ids):
                raise ValueError(f"stop_token_ids must be a list of integers >= 0 or None, got {self.stop_token_ids!r}")
            if len(set(self.stop_token_ids)) > MAX_STOP_TOKEN_IDS:
                raise ValueError(f"stop_token_ids holds {len(set(self.stop_token_ids))} distinct ids: at most {MAX_STOP_TOKEN_IDS}")
        if isinstance(self.min_tokens, bool) or not isinstance(self.min_tokens, int) or self.min_tokens < 0:
            raise ValueError(f"min_tokens must be an integer >= 0 (0 = off), got {self.min_tokens!r}")
        if self.min_tokens > self.max_new_tokens:
            raise ValueError(f"min_tokens = {self.min_tokens} exceeds max_new_tokens = {self.max_new_tokens}")
        if self.allowed_token_ids is not None:
            if (not isinstance(self.allowed_token_ids, (list, tuple)) or not self.allowed_token_ids
                    or not all(_is_id(t) for t in self.allowed_token_ids)):
                raise ValueError(f"allowed_token_ids must be a non-empty list of integers >= 0 or None, got {self.allowed_token_ids!r}")
        if self.bad_words_ids is not None:
            if not isinstance(self.bad_words_ids, (list, tuple)) or not all(
                    isinstance(w, (list, tuple)) and w and all(_is_id(t) for t in w) for w in self.bad_words_ids):
                raise ValueError(f"bad_words_ids must be a list of non-empty lists of integers >= 0 or None, got {self.bad_words_ids!r}")
            if len(self.bad_words_ids) > MAX_BAD_WORDS:
                raise ValueError(f"bad_words_ids holds {len(self.bad_words_ids)} words: at most {MAX_BAD_WORDS}")
            longest = max((len(w) for w in self.bad_words_ids), default=0)
            if longest > MAX_BAD_WORD_LEN:
                raise ValueError(f"bad_words_ids holds a word of {longest} tokens: at most {MAX_BAD_WORD_LEN}")
            total = sum(len(w) for w in self.bad_words_ids)
            if total > MAX_BAD_WORD_TOKENS:
                raise ValueError(f"bad_words_ids holds {total} tokens in all: at most {MAX_BAD_WORD_TOKENS}")
        if self.allowed_token_ids is not None:      # what is empty whatever the context; the EOS half is LLMEngine.add_request's
            left = set(self.allowed_token_ids) - {w[0] for w in self.bad_words_ids or () if len(w) == 1}
            if not left:
                raise ValueError("allowed_token_ids leaves nothing to generate: every id is also a one-token entry of bad_words_ids")
            if self.min_tokens > 0 and not left - set(self.stop_token_ids or ()):
                raise ValueError("allowed_token_ids leaves nothing to generate before min_tokens: every id that is not a one-token "
                                 "entry of bad_words_ids is in stop_token_ids")

        if self.lora is not None and (not isinstance(self.lora, str) or not self.lora):
            raise ValueError(f"lora must be None (off) or the non-empty name of a registered adapter, got {self.lora!r}")
        if self.guided_automaton is not None and self.guided_choice_ids is not None:
            raise ValueError("guided_automaton and guided_choice_ids cannot both be given: a request follows one guide")
        if self.guided_automaton is not None and not isinstance(self.guided_automaton, TokenAutomaton):
            raise ValueError(f"guided_automaton must be a TokenAutomaton or None, got {type(self.guided_automaton).__name__}")
        if self.guided_choice_ids is not None:
            if self.ignore_eos:
                raise ValueError("guided_choice_ids cannot go with ignore_eos=True: a choice ends on the EOS, so it could never end")
            # the shape and the limits, which do not depend on the EOS; LLMEngine.add_request builds the automaton the request follows,
            # so the trie is built here only where the tokens' count alone does not settle the limits
            check_choices(self.guided_choice_ids, "guided_choice_ids", trie=False)

    @property
    def active_guides(self) -> list[str]:
        """Names of the guided-decoding parameters that are switched on (at most one)."""
        return [n for n, on in (("guided_automaton", self.guided_automaton is not None),
                                ("guided_choice_ids", self.guided_choice_ids is not None)) if on]

    @property
    def active_penalties(self) -> list[str]:
        """Names of the penalty parameters that are switched on."""
        return [n for n, on in (("repetition_penalty", self.repetition_penalty != 1.0), ("presence_penalty", self.presence_penalty != 0.0),
                                ("frequency_penalty", self.frequency_penalty != 0.0), ("logit_bias", bool(self.logit_bias))) if on]

    @property
    def active_constraints(self) -> list[str]:
        """Names of the parameters that need the constraint kernel (stop_token_ids alone is host work and is not among them)."""
        return [n for n, on in (("min_tokens", self.min_tokens > 0), ("allowed_token_ids", self.allowed_token_ids is not None),
                                ("bad_words_ids", bool(self.bad_words_ids))) if on]

    @property
    def active_filters(self) -> list[str]:
        """Names of the truncation parameters that are switched on."""
        return [n for n, on in (("top_k", self.top_k > 0), ("top_p", self.top_p < 1.0), ("min_p", self.min_p > 0.0)) if on]
