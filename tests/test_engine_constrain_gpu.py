"""min_tokens / allowed_token_ids / bad_words_ids through the whole engine on the GPU, with the tiny pairs and the helpers of
tests/test_engine_penalty_gpu.py: autoregressive decoding, synchronous speculation with JIT and asynchronous speculation over the
in-process loopback.

  * allowed_token_ids of eight ids: every emitted token is in the set, at temperature 0 and at 0.8, in every mode;
  * min_tokens = 8 with the EOS set to a token the plain greedy stream emits early: the stream is the plain one up to that position, at
    least 8 long, and ends on the EOS only from output token 8 on;
  * bad_words_ids with the bigram (t3, t4) of the plain greedy stream: identical for four tokens, different at the fifth, never the
    bigram -- and in the speculative modes t4 is decided by a verify row whose predecessor t3 was speculated in the same round, so it
    fails if row j ignores the extras;
  * greedy constrained streams agree across the three modes;
  * speculative sampling stays exact under a mask plus bad words (two-sample chi-square of the temperature file, same bar, after two
    autoregressive samples passed it against each other; seeded, so the run is reproducible);
  * a same-model draft under synchronous speculation still gets nearly everything accepted: the draft chain is constrained like the target;
  * a default sequence beside a constrained one produces the stream it produces alone;
  * default SamplingParams launch no constrain kernel and create no constrain graph."""
from contextlib import contextmanager

import pytest
import torch

from tests.test_engine_filter_gpu import K, PROMPT2, engine
from tests.test_engine_temperature_gpu import PROMPT, cfgs, perturbed_pair, two_sample_ok

pytestmark = pytest.mark.gpu

MODES = ["ar", "sync", "async"]
ALLOWED = [3, 17, 42, 64, 77, 90, 101, 127]


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


def sp(**kw):
    from ssd_amd.sampling_params import SamplingParams
    return SamplingParams(**dict(dict(temperature=0, ignore_eos=True), **kw))


def streams(eng, prompts, params):
    out, m = eng.generate(prompts, params, use_tqdm=False)
    return [o["token_ids"] for o in out], m


@contextmanager
def eos_set(eng, eos):
    """The engine's EOS for the length of a test (the scheduler keeps its own copy; the runners read the config)."""
    saved = eng.config.eos, eng.scheduler.eos
    eng.config.eos = eng.scheduler.eos = eos
    try:
        yield
    finally:
        eng.config.eos, eng.scheduler.eos = saved


@pytest.mark.parametrize("mode", MODES)
def test_allowed_token_ids_confine_every_token_to_the_set(engines, mode):
    eng = engines[mode]
    plain, _ = streams(eng, [PROMPT, PROMPT2], sp(max_new_tokens=16))
    assert any(t not in ALLOWED for s in plain for t in s)
    for temp in (0, 0.8):
        got, m = streams(eng, [PROMPT, PROMPT2, PROMPT, PROMPT2], sp(temperature=temp, max_new_tokens=16, allowed_token_ids=ALLOWED))
        assert all(len(s) == 16 and set(s) <= set(ALLOWED) for s in got), (temp, got)
        if temp:
            assert len({t for s in got for t in s}) > 1 and len({tuple(s) for s in got}) > 1          # still sampling
        if mode != "ar":
            lens = m["accepted_suffix_lens_with_recovery"]
            print(mode, f"temperature {temp}: mean accepted (+recovery) under 8 allowed ids: {sum(lens) / len(lens):.3f}")


@pytest.mark.parametrize("mode", MODES)
def test_min_tokens_holds_the_eos_back(engines, mode):
    eng = engines[mode]
    plain, _ = streams(eng, [PROMPT], sp(max_new_tokens=24))
    plain = plain[0]
    i = next(i for i in range(1, 6) if plain[i] not in plain[:i])          # an early token, first met at output position i
    eos = plain[i]
    with eos_set(eng, eos):
        cut, _ = streams(eng, [PROMPT], sp(max_new_tokens=24, ignore_eos=False))
        assert cut[0] == plain[:i + 1]          # without min_tokens the request ends there
        got, _ = streams(eng, [PROMPT], sp(max_new_tokens=24, ignore_eos=False, min_tokens=8))
        got = got[0]
        print(mode, "eos", eos, "at", i, "plain", plain, "min_tokens=8", got)
        assert got[:i] == plain[:i] and got[i] != eos          # the plain stream up to the position of the EOS, then something else
        assert len(got) >= 8 and eos not in got[:8]
        assert eos not in got[:-1]          # it may end the stream (from output token 8 on), nothing else
        assert len(got) == 24 or got[-1] == eos
        # the same through stop_token_ids under ignore_eos: the stop id is held back just so, and reported when it ends the request
        out, _ = eng.generate([PROMPT], sp(max_new_tokens=24, min_tokens=8, stop_token_ids=[eos]), use_tqdm=False)
        assert out[0]["token_ids"] == got and out[0]["stop_reason"] == (eos if got[-1] == eos else None)


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
def test_a_banned_bigram_never_appears_and_straddles_a_verify_row(engines, mode):
    eng = engines[mode]
    # the first prompt whose output token 4 a verify row past the first decides (where the draft's acceptances fall depends on the prompt)
    for prompt in [PROMPT, PROMPT2] + [[(a * j + b) % 128 for j in range(9)] for a, b in ((3, 2), (11, 5), (13, 7), (9, 4), (17, 1), (19, 8))]:
        plain, m = streams(eng, [prompt], sp(max_new_tokens=24))
        plain = plain[0]
        row = 0 if mode == "ar" else _row_that_decides(m["accepted_suffix_lens_with_recovery"], 4)
        print(mode, "prompt", prompt, "accepted lengths", m["accepted_suffix_lens_with_recovery"][:4], "row", row)
        if mode == "ar" or row >= 1:
            break
    else:
        raise AssertionError("output token 4 is decided by row 0 of its round for every prompt: no straddle to test")
    t3, t4 = plain[3], plain[4]
    assert (t3, t4) not in zip(plain[:4], plain[1:4])          # the bigram's first occurrence is the one at positions 3, 4
    print(mode, "bigram", (t3, t4), "decided by verify row", row)
    got, _ = streams(eng, [prompt], sp(max_new_tokens=24, bad_words_ids=[[t3, t4]]))
    got = got[0]
    assert len(got) == 24 and got[:4] == plain[:4] and got[4] != t4, (plain, got)
    assert (t3, t4) not in zip(got, got[1:]), got


def test_greedy_constrained_streams_agree_across_modes(engines):
    prompts = [PROMPT, PROMPT2, PROMPT, PROMPT2]
    plain, _ = streams(engines["ar"], prompts, sp(max_new_tokens=24))
    words = [[plain[0][3], plain[0][4]], [plain[1][1]], [plain[1][5], plain[1][6], plain[1][7]]]
    params = sp(max_new_tokens=24, allowed_token_ids=list(range(0, 128, 2)) + plain[0][:8] + plain[1][:8], bad_words_ids=words)
    ar, _ = streams(engines["ar"], prompts, params)
    assert all(len(s) == 24 for s in ar) and ar != plain
    for mode in ("sync", "async"):
        got, m = streams(engines[mode], prompts, params)
        lens = m["accepted_suffix_lens_with_recovery"]
        print(mode, "mean accepted (+recovery) under mask + bad words:", sum(lens) / len(lens))
        assert got == ar, mode


N_NEW = 6
CON = dict(temperature=0.8, allowed_token_ids=[t for t in range(128) if t % 3], bad_words_ids=[[5], [7, 8], [1, 2], [10, 11, 13]])


def draw_seeded(eng, rounds, per_round, n_new, seed0):
    """tests/test_engine_temperature_gpu.py draw() with a seed per request (seed0 + its number), so the sample is reproducible."""
    toks, lens = [], []
    for r in range(rounds):
        params = [sp(max_new_tokens=n_new, seed=seed0 + r * per_round + i, **CON) for i in range(per_round)]
        out, m = eng.generate([PROMPT] * per_round, params, use_tqdm=False)
        toks.extend(o["token_ids"][:n_new] for o in out)
        lens.extend(m.get("accepted_suffix_lens_with_recovery", []))
    return torch.tensor(toks), lens


def _obeys(sample):
    ok = set(CON["allowed_token_ids"]) - {5}
    for row in sample.tolist():
        assert set(row) <= ok, row
        for w in CON["bad_words_ids"][1:]:
            assert all(tuple(row[i:i + len(w)]) != tuple(w) for i in range(len(row))), (w, row)


@pytest.fixture(scope="module")
def ar_sample(engines):
    """Autoregressive continuations under the constraints, drawn once for the sync and the async comparison; a second, independent
    draw (other seeds) must pass the bar against the first before the bar is used on the speculative engines."""
    t, _ = cfgs()
    a, _ = draw_seeded(engines["ar"], 40, 48, N_NEW, 1_000_000)
    b, _ = draw_seeded(engines["ar"], 40, 48, N_NEW, 2_000_000)
    assert a[:, 1].unique().numel() >= 4, "degenerate test distribution"
    assert not torch.equal(a, b)
    _obeys(a)
    for pos in range(1, N_NEW):
        two_sample_ok(a[:, pos], b[:, pos], t.vocab_size, f"ar against ar, constrained: marginal of generated position {pos}")
    return a


def test_sync_speculation_matches_autoregressive_sampling_under_constraints(engines, ar_sample):
    t, _ = cfgs()
    s, lens = draw_seeded(engines["sync"], 40, 48, N_NEW, 3_000_000)
    print("sync: mean accepted (+recovery)", sum(lens) / len(lens))
    assert min(lens) < K + 1 and max(lens) == K + 1          # rejections and fully accepted rounds: both branches exercised
    _obeys(s)
    for pos in range(1, N_NEW):
        two_sample_ok(ar_sample[:, pos], s[:, pos], t.vocab_size, f"sync, constrained: marginal of generated position {pos}")


def test_async_speculation_matches_autoregressive_sampling_under_constraints(engines, ar_sample):
    t, _ = cfgs()
    s, lens = draw_seeded(engines["async"], 40, 8, N_NEW, 4_000_000)
    print("async: mean accepted (+recovery)", sum(lens) / len(lens))
    assert min(lens) < K + 1 and max(lens) == K + 1
    _obeys(s)
    for pos in range(1, N_NEW):
        two_sample_ok(ar_sample[:, pos], s[:, pos], t.vocab_size, f"async, constrained: marginal of generated position {pos}")


@pytest.fixture(scope="module")
def same_model_sync(gpu):
    return engine("sync", B=8, weights_seed=0, draft_weights_seed=0)


def test_same_model_draft_under_allowed_token_ids_accepts_nearly_everything(same_model_sync):
    """The existing same-model bar (mean accepted length with recovery above 3.8 of 4): it holds only if the draft chain is constrained
    like the target -- an unconstrained draft proposes tokens outside the set, which the target rejects."""
    lens = []
    for _ in range(4):
        out, m = same_model_sync.generate([PROMPT] * 8, sp(temperature=0.9, allowed_token_ids=ALLOWED, max_new_tokens=24), use_tqdm=False)
        lens += m["accepted_suffix_lens_with_recovery"]
        assert all(set(o["token_ids"]) <= set(ALLOWED) for o in out)
    print(f"sync: mean accepted (+recovery) under 8 allowed ids: {sum(lens) / len(lens):.3f} over {len(lens)} rounds")
    assert sum(lens) / len(lens) > 3.8, lens
    assert len({tuple(o["token_ids"]) for o in out}) > 1          # still sampling: rows draw independently


@pytest.mark.parametrize("mode", MODES)
def test_default_sequence_beside_a_constrained_one_keeps_its_stream(engines, mode):
    eng = engines[mode]
    con = sp(max_new_tokens=16, allowed_token_ids=list(range(1, 128, 2)), bad_words_ids=[[9], [3, 5]], min_tokens=4)
    alone, _ = streams(eng, [PROMPT2], sp(max_new_tokens=16))
    con_alone, _ = streams(eng, [PROMPT], con)
    mixed, _ = eng.generate([PROMPT, PROMPT2], [con, sp(max_new_tokens=16)], use_tqdm=False)
    assert mixed[1]["token_ids"] == alone[0]
    assert mixed[0]["token_ids"] == con_alone[0] and all(t % 2 == 1 and t != 9 for t in con_alone[0])
    assert "stop_reason" not in mixed[0] and "stop_reason" not in mixed[1]


def _has_con(name: str) -> bool:
    """The graph's Sampling suffix carries the constraint letter (behind the body's name: "decode_chain" has a "_c" of its own)."""
    for body in ("decode_chain", "decode_deposit", "decode", "verify_logits", "verify", "tree", "glue_fork", "prefill"):
        if name.startswith(body):
            return "_c" in name[len(body):]
    raise AssertionError(name)


def test_default_sampling_params_launch_no_constrain_kernel_and_make_no_constrain_graph(engines, same_model_sync):
    from ssd_amd.hip import constrain_ops
    engs = list(engines.values()) + [same_model_sync]

    def keys():
        out = set()
        for e in engs:
            for r in (e.model_runner, e.draft_runner):
                if r is not None:
                    out |= {(id(r), k[0]) for k in r.graphs}
        return out
    n0, k0 = constrain_ops.LAUNCHES, keys()
    for e in engs:
        for temp in (0, 0.7):
            out, _ = e.generate([PROMPT] * 4, sp(temperature=temp, max_new_tokens=12, stop_token_ids=[128]), use_tqdm=False)
            assert all(len(o["token_ids"]) == 12 and o["stop_reason"] is None for o in out)          # stop ids alone: host work
    assert constrain_ops.LAUNCHES == n0
    fresh = {name for _, name in keys() - k0}
    assert not any(_has_con(name) for name in fresh), fresh
    assert not any(_has_con(name) for _, name in keys()) or n0 > 0          # constrain graphs exist only if a constrained request ran
    out, _ = engines["sync"].generate([PROMPT] * 4, sp(max_new_tokens=12, min_tokens=2), use_tqdm=False)
    assert constrain_ops.LAUNCHES > n0          # ... and the counter does count
    assert any(_has_con(name) for _, name in keys())
