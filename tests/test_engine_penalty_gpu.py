"""repetition_penalty / presence_penalty / frequency_penalty / logit_bias through the whole engine on the GPU, with the tiny pairs and the
helpers of tests/test_engine_filter_gpu.py and tests/test_engine_temperature_gpu.py: autoregressive decoding, synchronous speculation
with JIT and asynchronous speculation over the in-process loopback.

  * a bias of +100 forces a token and a bias of -100 bans one, in every mode;
  * presence_penalty = 1000 at temperature 0 gives 32 distinct tokens where the plain request repeats itself: it fails if a verify row
    ignores the tokens speculated in front of it in the same round, or a chain step the chain's own tokens;
  * the greedy stream under repetition_penalty = 1.3 is the same stream in every mode;
  * speculative sampling stays exact under penalties (two-sample chi-square of the temperature file, same bar, after two
    autoregressive samples passed it against each other);
  * a same-model draft under synchronous speculation still gets nearly everything accepted: the draft chain is penalised like the target;
  * a default sequence beside a penalised one produces the stream it produces alone;
  * default SamplingParams launch no penalty kernel and create no penalty graph."""
import pytest
import torch

from tests.test_engine_filter_gpu import K, PROMPT2, engine
from tests.test_engine_temperature_gpu import PROMPT, cfgs, draw, perturbed_pair, two_sample_ok

pytestmark = pytest.mark.gpu

MODES = ["ar", "sync", "async"]


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


@pytest.mark.parametrize("mode", MODES)
def test_logit_bias_forces_and_bans_a_token(engines, mode):
    eng = engines[mode]
    plain, _ = streams(eng, [PROMPT, PROMPT2], sp(max_new_tokens=16))
    t = 77
    assert any(tok != t for s in plain for tok in s)
    forced, _ = streams(eng, [PROMPT, PROMPT2], sp(max_new_tokens=16, logit_bias={t: 100}))
    assert forced == [[t] * 16] * 2
    for prompt, base in zip((PROMPT, PROMPT2), plain):
        first = base[0]
        banned, _ = streams(eng, [prompt], sp(max_new_tokens=16, logit_bias={first: -100}))
        assert len(banned[0]) == 16 and first not in banned[0], (first, banned[0])


@pytest.mark.parametrize("mode", MODES)
def test_presence_penalty_1000_gives_32_distinct_tokens(engines, mode):
    eng = engines[mode]
    plain, _ = streams(eng, [PROMPT, PROMPT2], sp(max_new_tokens=32))
    print(mode, "distinct tokens of the plain streams:", [len(set(s)) for s in plain])
    assert all(len(set(s)) < 32 for s in plain), "the plain request does not repeat itself: the test below would show nothing"
    got, m = streams(eng, [PROMPT, PROMPT2], sp(max_new_tokens=32, presence_penalty=1000))
    assert all(len(s) == 32 and len(set(s)) == 32 for s in got), got
    if mode != "ar":        # speculated tokens were accepted along the way: rows past the first did decide tokens
        lens = m["accepted_suffix_lens_with_recovery"]
        print(mode, "mean accepted (+recovery) under presence_penalty=1000:", sum(lens) / len(lens))


def test_greedy_streams_under_repetition_penalty_agree_across_modes(engines):
    prompts = [PROMPT, PROMPT2, PROMPT, PROMPT2]
    params = sp(max_new_tokens=24, repetition_penalty=1.3)
    ar, _ = streams(engines["ar"], prompts, params)
    assert all(len(s) == 24 for s in ar)
    plain, _ = streams(engines["ar"], prompts, sp(max_new_tokens=24))
    assert ar != plain          # the penalty does change the stream
    for mode in ("sync", "async"):
        got, m = streams(engines[mode], prompts, params)
        lens = m["accepted_suffix_lens_with_recovery"]
        print(mode, "mean accepted (+recovery) under repetition_penalty=1.3:", sum(lens) / len(lens))
        assert got == ar, mode


N_NEW = 6
PEN = dict(temperature=0.8, repetition_penalty=1.2, frequency_penalty=0.5)


@pytest.fixture(scope="module")
def ar_sample(engines):
    """Autoregressive continuations under the penalties, drawn once for the sync and the async comparison; a second, independent draw
    (the device RNG has moved on) must pass the bar against the first before the bar is used on the speculative engines."""
    t, _ = cfgs()
    a, _ = draw(engines["ar"], sp(max_new_tokens=N_NEW, **PEN), 40, 48, N_NEW)
    b, _ = draw(engines["ar"], sp(max_new_tokens=N_NEW, **PEN), 40, 48, N_NEW)
    assert a[:, 1].unique().numel() >= 4, "degenerate test distribution"
    assert not torch.equal(a, b)
    for pos in range(1, N_NEW):
        two_sample_ok(a[:, pos], b[:, pos], t.vocab_size, f"ar against ar, penalised: marginal of generated position {pos}")
    return a


def test_sync_speculation_matches_autoregressive_sampling_under_penalties(engines, ar_sample):
    t, _ = cfgs()
    s, lens = draw(engines["sync"], sp(max_new_tokens=N_NEW, **PEN), 40, 48, N_NEW)
    print("sync: mean accepted (+recovery)", sum(lens) / len(lens))
    assert min(lens) < K + 1 and max(lens) == K + 1          # rejections and fully accepted rounds: both branches exercised
    for pos in range(1, N_NEW):
        two_sample_ok(ar_sample[:, pos], s[:, pos], t.vocab_size, f"sync, penalised: marginal of generated position {pos}")


def test_async_speculation_matches_autoregressive_sampling_under_penalties(engines, ar_sample):
    t, _ = cfgs()
    s, lens = draw(engines["async"], sp(max_new_tokens=N_NEW, **PEN), 40, 8, N_NEW)
    print("async: mean accepted (+recovery)", sum(lens) / len(lens))
    assert min(lens) < K + 1 and max(lens) == K + 1
    for pos in range(1, N_NEW):
        two_sample_ok(ar_sample[:, pos], s[:, pos], t.vocab_size, f"async, penalised: marginal of generated position {pos}")


@pytest.fixture(scope="module")
def same_model_sync(gpu):
    return engine("sync", B=8, weights_seed=0, draft_weights_seed=0)


def test_same_model_draft_under_repetition_penalty_accepts_nearly_everything(same_model_sync):
    """The existing same-model bar (mean accepted length with recovery above 3.8 of 4): it holds only if the draft chain is penalised
    like the target, its own tokens of the round included."""
    lens = []
    for _ in range(4):
        out, m = same_model_sync.generate([PROMPT] * 8, sp(temperature=0.9, repetition_penalty=1.2, max_new_tokens=24), use_tqdm=False)
        lens += m["accepted_suffix_lens_with_recovery"]
    print(f"sync: mean accepted (+recovery) under repetition_penalty=1.2: {sum(lens) / len(lens):.3f} over {len(lens)} rounds")
    assert sum(lens) / len(lens) > 3.8, lens
    assert len({tuple(o["token_ids"]) for o in out}) > 1          # still sampling: rows draw independently


@pytest.mark.parametrize("mode", MODES)
def test_default_sequence_beside_a_penalised_one_keeps_its_stream(engines, mode):
    eng = engines[mode]
    alone, _ = streams(eng, [PROMPT2], sp(max_new_tokens=16))
    pen_alone, _ = streams(eng, [PROMPT], sp(max_new_tokens=16, repetition_penalty=1.5, presence_penalty=0.7, logit_bias={3: 4.0}))
    mixed, _ = eng.generate([PROMPT, PROMPT2], [sp(max_new_tokens=16, repetition_penalty=1.5, presence_penalty=0.7, logit_bias={3: 4.0}),
                                                sp(max_new_tokens=16)], use_tqdm=False)
    assert mixed[1]["token_ids"] == alone[0]
    assert mixed[0]["token_ids"] == pen_alone[0]


def test_default_sampling_params_launch_no_penalty_kernel_and_make_no_penalty_graph(engines, same_model_sync):
    from ssd_amd.hip import penalty_ops
    engs = list(engines.values()) + [same_model_sync]

    def keys():
        out = set()
        for e in engs:
            for r in (e.model_runner, e.draft_runner):
                if r is not None:
                    out |= {(id(r), k[0]) for k in r.graphs}
        return out
    n0, k0 = penalty_ops.LAUNCHES, keys()
    for e in engs:
        for temp in (0, 0.7):
            out, _ = e.generate([PROMPT] * 4, sp(temperature=temp, max_new_tokens=12), use_tqdm=False)
            assert all(len(o["token_ids"]) == 12 for o in out)
    assert penalty_ops.LAUNCHES == n0
    fresh = {name for _, name in keys() - k0}
    assert not any(name.endswith("_p") for name in fresh), fresh
    assert not any(name.endswith("_p") for _, name in keys()) or n0 > 0          # penalty graphs exist only if a penalised request ran
    out, _ = engines["sync"].generate([PROMPT] * 4, sp(max_new_tokens=12, repetition_penalty=1.1), use_tqdm=False)
    assert penalty_ops.LAUNCHES > n0          # ... and the counter does count
    assert any(name.endswith("_p") for _, name in keys())
