"""guided_automaton / guided_choice_ids through the whole engine on the GPU, with the tiny pairs and the helpers of
tests/test_engine_constrain_gpu.py: autoregressive decoding, synchronous speculation with JIT and asynchronous speculation over the
in-process loopback.

  1. guided_choice_ids with three choices (two share their first token) and the EOS set to a token of the vocabulary: every output is
     one of the choices followed by the EOS, at temperature 0 and at 0.8, in every mode;
  2. the automaton "anything; after t3 anything but t4", built from the plain greedy stream, gives the stream of
     bad_words_ids=[[t3, t4]] -- and in the speculative modes t4 is decided by a verify row whose predecessor t3 was speculated in the same
     round, so it fails if row j ignores the extras;
  3. the one-state automaton with self-loops on ALLOWED gives the stream of allowed_token_ids=ALLOWED, at temperature 0 and, with the
     same seed, at 0.8: the banned bits are identical, so the tokens must be;
  4. greedy guided streams agree across the three modes;
  5. speculative sampling stays exact under an automaton (two-sample chi-square of the temperature file, same bar, after two
     autoregressive samples passed it against each other; seeded, so the run is reproducible);
  6. a same-model draft under synchronous speculation still gets nearly everything accepted: the draft chain walks the automaton too;
  7. a default sequence beside a guided one produces the stream it produces alone, and default SamplingParams launch no guide kernel
     and create no guide graph;
  8. a guided request that takes the batch row of a finished guided request with another automaton is guided by its own."""
import pytest
import torch

from tests.test_engine_filter_gpu import K, PROMPT2, engine
from tests.test_engine_temperature_gpu import PROMPT, cfgs, perturbed_pair, two_sample_ok
from tests.test_engine_constrain_gpu import ALLOWED, MODES, eos_set, sp, streams

pytestmark = pytest.mark.gpu

V = 128
EOS = 100
CHOICES = [[10, 20, 30], [10, 21, 31, 41], [50, 60, 70]]


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssd_amd.hip import ops
    return ops


@pytest.fixture(scope="module")
def engines(gpu):
    """One engine per decoding mode over the correlated pair (draft = target + 3 % noise), shared by the tests below."""
    t, factory = perturbed_pair(0.03)
    return {"ar": engine("ar", factory), "sync": engine("sync", factory), "async": engine("async", factory, B=8)}


def residues():
    """Three states: at state s every token t with t % 3 != s is allowed and leads to state t % 3 (so no two neighbours of the output are
    congruent, and the first token is not divisible by 3); 85 or 86 edges per state, no default."""
    from ssd_amd.guide import TokenAutomaton
    return TokenAutomaton(3, 0, {s: {t: t % 3 for t in range(V) if t % 3 != s} for s in range(3)})


def obeys(automaton, row):
    return automaton.walk(automaton.start, row) != -1


# ---- 1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_every_output_is_one_of_the_choices_followed_by_the_eos(engines, mode):
    eng = engines[mode]
    prompts = [PROMPT, PROMPT2, PROMPT, PROMPT2, PROMPT[:5], PROMPT2[:6]]
    want = {tuple(c + [EOS]) for c in CHOICES}
    with eos_set(eng, EOS):
        for temp in (0, 0.8):
            got, m = streams(eng, prompts, sp(temperature=temp, max_new_tokens=16, ignore_eos=False, guided_choice_ids=CHOICES))
            assert all(tuple(s) in want for s in got), (temp, got)
            if mode != "ar":
                lens = m["accepted_suffix_lens_with_recovery"]
                print(mode, f"temperature {temp}: mean accepted (+recovery) under the choice automaton: {sum(lens) / len(lens):.3f}")


# ---- 2 -------------------------------------------------------------------------------------------------------------------
def _row_that_decides(lens, i):
    """The verify row that produced output token i of a single request, from the accepted lengths (with recovery) of its rounds: round
    r commits stream[c : c + L]; an accepted draft token at c < i < c + L was checked by row i - c - 1, the recovery token at c + L comes
    from row L - 1.  Output token 0 is the prefill's."""
    c = 0
    for L in lens:
        if c < i <= c + L:
            return i - c - 1
        c += L
    raise AssertionError((lens, i))


@pytest.mark.parametrize("mode", MODES)
def test_the_bigram_automaton_gives_the_stream_of_the_bad_word_and_straddles_a_verify_row(engines, mode):
    from ssd_amd.guide import TokenAutomaton
    eng = engines[mode]
    # the first prompt whose output token 4 a verify row past the first decides (where the draft's acceptances fall depends on the prompt)
    for prompt in [PROMPT, PROMPT2] + [[(a * j + b) % 128 for j in range(9)] for a, b in ((3, 2), (11, 5), (13, 7), (9, 4), (17, 1), (19, 8))]:
        plain, m = streams(eng, [prompt], sp(max_new_tokens=24))
        plain = plain[0]
        row = 0 if mode == "ar" else _row_that_decides(m["accepted_suffix_lens_with_recovery"], 4)
        if mode == "ar" or row >= 1:
            break
    else:
        raise AssertionError("output token 4 is decided by row 0 of its round for every prompt: no straddle to test")
    t3, t4 = plain[3], plain[4]
    assert (t3, t4) not in zip(plain[:4], plain[1:4])          # the bigram's first occurrence is the one at positions 3, 4
    print(mode, "bigram", (t3, t4), "decided by verify row", row)
    # state 0: anything, t3 leads to state 1; state 1: anything but t4, t3 stays
    after = {t3: 1}
    after[t4] = -1
    auto = TokenAutomaton(2, 0, {0: {t3: 1}, 1: after}, {0: 0, 1: 0})
    got, _ = streams(eng, [prompt], sp(max_new_tokens=24, guided_automaton=auto))
    words, _ = streams(eng, [prompt], sp(max_new_tokens=24, bad_words_ids=[[t3, t4]]))
    got, words = got[0], words[0]
    assert len(got) == 24 and got[:4] == plain[:4] and got[4] != t4, (plain, got)          # t3 was among the deciding row's extras
    assert (t3, t4) not in zip(got, got[1:]), got
    assert got == words, (got, words)


# ---- 3 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_the_self_loop_automaton_gives_the_stream_of_allowed_token_ids(engines, mode):
    from ssd_amd.guide import TokenAutomaton
    eng = engines[mode]
    auto = TokenAutomaton(1, 0, {0: {t: 0 for t in ALLOWED}})
    prompts = [PROMPT, PROMPT2, PROMPT, PROMPT2]
    for temp in (0, 0.8):
        seeds = [dict(seed=500 + i) if temp else {} for i in range(len(prompts))]
        mask, _ = streams(eng, prompts, [sp(temperature=temp, max_new_tokens=16, allowed_token_ids=ALLOWED, **s) for s in seeds])
        got, _ = streams(eng, prompts, [sp(temperature=temp, max_new_tokens=16, guided_automaton=auto, **s) for s in seeds])
        assert all(len(s) == 16 and set(s) <= set(ALLOWED) for s in got), (temp, got)
        assert got == mask, (temp, got, mask)
        if temp:
            assert len({tuple(s) for s in got}) > 1


# ---- 4 -------------------------------------------------------------------------------------------------------------------
def test_greedy_guided_streams_agree_across_modes(engines):
    prompts = [PROMPT, PROMPT2, PROMPT[:6], PROMPT2[:7]]
    auto = residues()
    plain, _ = streams(engines["ar"], prompts, sp(max_new_tokens=24))
    params = sp(max_new_tokens=24, guided_automaton=auto)
    ar, _ = streams(engines["ar"], prompts, params)
    assert all(len(s) == 24 and obeys(auto, s) for s in ar) and ar != plain and not all(obeys(auto, s) for s in plain)
    with eos_set(engines["ar"], EOS):
        ar_choice, _ = streams(engines["ar"], prompts, sp(max_new_tokens=16, ignore_eos=False, guided_choice_ids=CHOICES))
    for mode in ("sync", "async"):
        got, m = streams(engines[mode], prompts, params)
        lens = m["accepted_suffix_lens_with_recovery"]
        print(mode, "mean accepted (+recovery) under the residue automaton:", sum(lens) / len(lens))
        assert got == ar, mode
        with eos_set(engines[mode], EOS):
            got, _ = streams(engines[mode], prompts, sp(max_new_tokens=16, ignore_eos=False, guided_choice_ids=CHOICES))
        assert got == ar_choice, mode


# ---- 5 -------------------------------------------------------------------------------------------------------------------
N_NEW = 6


def draw_seeded(eng, rounds, per_round, n_new, seed0):
    """tests/test_engine_temperature_gpu.py draw() with a seed per request (seed0 + its number), so the sample is reproducible."""
    auto = residues()
    toks, lens = [], []
    for r in range(rounds):
        params = [sp(max_new_tokens=n_new, temperature=0.8, guided_automaton=auto, seed=seed0 + r * per_round + i) for i in range(per_round)]
        out, m = eng.generate([PROMPT] * per_round, params, use_tqdm=False)
        toks.extend(o["token_ids"][:n_new] for o in out)
        lens.extend(m.get("accepted_suffix_lens_with_recovery", []))
    sample = torch.tensor(toks)
    assert all(obeys(auto, row) for row in sample.tolist())
    return sample, lens


@pytest.fixture(scope="module")
def ar_sample(engines):
    """Autoregressive continuations under the automaton, drawn once for the sync and the async comparison; a second, independent draw
    (other seeds) must pass the bar against the first before the bar is used on the speculative engines."""
    t, _ = cfgs()
    a, _ = draw_seeded(engines["ar"], 40, 48, N_NEW, 1_000_000)
    b, _ = draw_seeded(engines["ar"], 40, 48, N_NEW, 2_000_000)
    assert a[:, 1].unique().numel() >= 4, "degenerate test distribution"
    assert not torch.equal(a, b)
    for pos in range(1, N_NEW):
        two_sample_ok(a[:, pos], b[:, pos], t.vocab_size, f"ar against ar, guided: marginal of generated position {pos}")
    return a


def test_sync_speculation_matches_autoregressive_sampling_under_an_automaton(engines, ar_sample):
    t, _ = cfgs()
    s, lens = draw_seeded(engines["sync"], 40, 48, N_NEW, 3_000_000)
    print("sync: mean accepted (+recovery)", sum(lens) / len(lens))
    assert min(lens) < K + 1 and max(lens) == K + 1          # rejections and fully accepted rounds: both branches exercised
    for pos in range(1, N_NEW):
        two_sample_ok(ar_sample[:, pos], s[:, pos], t.vocab_size, f"sync, guided: marginal of generated position {pos}")


def test_async_speculation_matches_autoregressive_sampling_under_an_automaton(engines, ar_sample):
    t, _ = cfgs()
    s, lens = draw_seeded(engines["async"], 40, 8, N_NEW, 4_000_000)
    print("async: mean accepted (+recovery)", sum(lens) / len(lens))
    assert min(lens) < K + 1 and max(lens) == K + 1
    for pos in range(1, N_NEW):
        two_sample_ok(ar_sample[:, pos], s[:, pos], t.vocab_size, f"async, guided: marginal of generated position {pos}")


# ---- 6 -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def same_model_sync(gpu):
    return engine("sync", B=8, weights_seed=0, draft_weights_seed=0)


def test_same_model_draft_under_an_automaton_accepts_nearly_everything(same_model_sync):
    """The existing same-model bar (mean accepted length with recovery above 3.8 of 4): it holds only if the draft chain walks the
    automaton like the target -- an unguided draft proposes tokens the state bans, which the target rejects."""
    auto = residues()
    lens = []
    for _ in range(4):
        out, m = same_model_sync.generate([PROMPT] * 8, sp(temperature=0.9, guided_automaton=auto, max_new_tokens=24), use_tqdm=False)
        lens += m["accepted_suffix_lens_with_recovery"]
        assert all(obeys(auto, o["token_ids"]) for o in out)
    print(f"sync: mean accepted (+recovery) under the residue automaton: {sum(lens) / len(lens):.3f} over {len(lens)} rounds")
    assert sum(lens) / len(lens) > 3.8, lens
    assert len({tuple(o["token_ids"]) for o in out}) > 1          # still sampling: rows draw independently


# ---- 7 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_default_sequence_beside_a_guided_one_keeps_its_stream(engines, mode):
    eng = engines[mode]
    auto = residues()
    guided = sp(max_new_tokens=16, guided_automaton=auto)
    alone, _ = streams(eng, [PROMPT2], sp(max_new_tokens=16))
    guided_alone, _ = streams(eng, [PROMPT], guided)
    mixed, _ = eng.generate([PROMPT, PROMPT2], [guided, sp(max_new_tokens=16)], use_tqdm=False)
    assert mixed[1]["token_ids"] == alone[0] and not obeys(auto, alone[0])
    assert mixed[0]["token_ids"] == guided_alone[0] and obeys(auto, guided_alone[0])
    assert set(mixed[0]) == set(mixed[1])          # no new output key


def _has_guide(name: str) -> bool:
    """The graph's Sampling suffix carries the guide letter."""
    for body in ("decode_chain", "decode_deposit", "decode", "verify_logits", "verify", "tree", "glue_fork", "prefill"):
        if name.startswith(body):
            return "_g" in name[len(body):]
    raise AssertionError(name)


def test_default_sampling_params_launch_no_guide_kernel_and_make_no_guide_graph(engines, same_model_sync):
    from ssd_amd.hip import guide_ops
    engs = list(engines.values()) + [same_model_sync]

    def keys():
        out = set()
        for e in engs:
            for r in (e.model_runner, e.draft_runner):
                if r is not None:
                    out |= {(id(r), k[0]) for k in r.graphs}
        return out
    n0, k0 = guide_ops.LAUNCHES, keys()
    for e in engs:
        for temp in (0, 0.7):
            out, _ = e.generate([PROMPT] * 4, sp(temperature=temp, max_new_tokens=12, min_tokens=2), use_tqdm=False)
            assert all(len(o["token_ids"]) == 12 for o in out)
    assert guide_ops.LAUNCHES == n0
    fresh = {name for _, name in keys() - k0}
    assert not any(_has_guide(name) for name in fresh), fresh
    assert not any(_has_guide(name) for _, name in keys()) or n0 > 0          # guide graphs exist only if a guided request ran
    out, _ = engines["sync"].generate([PROMPT] * 4, sp(max_new_tokens=12, guided_automaton=residues()), use_tqdm=False)
    assert guide_ops.LAUNCHES > n0          # ... and the counter does count
    assert any(_has_guide(name) for _, name in keys())


# ---- 8 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_a_request_that_inherits_a_batch_row_is_guided_by_its_own_automaton(engines, mode):
    from ssd_amd.guide import TokenAutomaton
    eng = engines[mode]
    evens = TokenAutomaton(1, 0, {0: {t: 0 for t in range(0, V, 2)}})
    odds = TokenAutomaton(1, 0, {0: {t: 0 for t in range(1, V, 2)}})
    odd_alone, _ = streams(eng, [PROMPT2], sp(max_new_tokens=20, guided_automaton=odds))
    # one call: the first request finishes after two tokens and the second moves up into its batch row
    got, _ = streams(eng, [PROMPT, PROMPT2], [sp(max_new_tokens=2, guided_automaton=evens), sp(max_new_tokens=20, guided_automaton=odds)])
    assert all(t % 2 == 0 for t in got[0]) and len(got[0]) == 2
    assert got[1] == odd_alone[0] and all(t % 2 == 1 for t in got[1]) and len(got[1]) == 20
    # two calls: the same row, one request after the other
    a, _ = streams(eng, [PROMPT2], sp(max_new_tokens=20, guided_automaton=evens))
    b, _ = streams(eng, [PROMPT2], sp(max_new_tokens=20, guided_automaton=odds))
    assert all(t % 2 == 0 for t in a[0]) and b == odd_alone
    # where the tables went: the prefill used the last slot, the decode (or verify) batch slot 0 -- so the prefill of an arriving
    # request does not evict the automaton of the sequence running in row 0 -- and both hold the last request's
    for r in (eng.model_runner, eng.draft_runner if mode == "sync" else None):
        if r is not None:
            assert "gd" in r.rules, sorted(r.rules)         # a runner that guided something has the rule object
            owner = r.rules["gd"].owner
            assert owner[0] is not None
            if not r.is_draft:          # (a draft's prefill token is never used, so it is not guided)
                assert owner[r.seq_cap - 1] == owner[0], owner
