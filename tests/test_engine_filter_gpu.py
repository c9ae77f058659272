"""top_k / top_p / min_p through the whole engine on the GPU, with the tiny pair of tests/test_engine_temperature_gpu.py: autoregressive
sampling, synchronous speculation with JIT and asynchronous speculation over the in-process loopback.

  * top_k = 1 at temperature 1.0 is greedy decoding: every mode reproduces its own temperature-0 stream token for token;
  * speculative sampling stays exact under truncation: with temperature 0.9, top_k 20, top_p 0.8 the sync and async streams have the
    distribution of autoregressive sampling with the same parameters (two-sample chi-square of that file, same bar);
  * the draft's q is truncated like the target's p: a same-model draft under top_p = 0.5 still gets nearly everything accepted
    (an unfiltered draft would propose tail tokens that the truncated target rejects with certainty);
  * a mixed batch: the greedy sequence stays greedy, and a filtered sequence's first token comes from the reference kept set
    (tests/filter_ref.py) of the prefill's own logits;
  * with default SamplingParams no filter is ever launched."""
import numpy as np
import pytest
import torch

from tests import filter_ref as R
from tests.test_engine_temperature_gpu import KW, PROMPT, cfgs, draw, perturbed_pair, two_sample_ok

pytestmark = pytest.mark.gpu

K = 3
PROMPT2 = [(7 * j + 3) % 128 for j in range(11)]


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssd_amd.hip import ops
    return ops


def engine(mode: str, factory=None, hf=None, B: int = 48, **extra):
    from ssd_amd.engine.llm_engine import LLMEngine
    t, _ = cfgs()
    hf = hf or t
    kw = dict(KW, **extra)
    if factory is not None:
        kw["runner_factory"] = factory
    if mode == "ar":
        return LLMEngine("t", hf_config=hf, max_num_seqs=B, **kw)
    spec = dict(draft="d", draft_hf_config=hf, speculate=True, speculate_k=K, jit_speculate=True)
    if mode == "sync":
        return LLMEngine("t", hf_config=hf, max_num_seqs=B, **spec, **kw)
    assert mode == "async"
    return LLMEngine("t", hf_config=hf, max_num_seqs=B, draft_async=True, async_fan_out=3, inprocess_draft=True, **spec, **kw)


@pytest.fixture(scope="module")
def engines(gpu):
    """One engine per decoding mode over the correlated pair (draft = target + 3 % noise), shared by the tests below."""
    t, factory = perturbed_pair(0.03)
    return {"ar": engine("ar", factory), "sync": engine("sync", factory), "async": engine("async", factory, B=8)}


@pytest.mark.parametrize("mode", ["ar", "sync", "async"])
def test_top_k_1_at_temperature_1_is_the_greedy_stream(engines, mode):
    from ssd_amd.sampling_params import SamplingParams
    eng = engines[mode]
    prompts = [PROMPT, PROMPT2, PROMPT, PROMPT2]
    greedy, _ = eng.generate(prompts, SamplingParams(temperature=0, max_new_tokens=24, ignore_eos=True), use_tqdm=False)
    top1, m = eng.generate(prompts, SamplingParams(temperature=1.0, top_k=1, max_new_tokens=24, ignore_eos=True), use_tqdm=False)
    assert [o["token_ids"] for o in top1] == [o["token_ids"] for o in greedy]
    assert all(len(o["token_ids"]) == 24 for o in top1)
    # the same temperature without the filter is not greedy: the equality above is the filter's doing
    free, _ = eng.generate(prompts, SamplingParams(temperature=1.0, max_new_tokens=24, ignore_eos=True), use_tqdm=False)
    assert [o["token_ids"] for o in free] != [o["token_ids"] for o in greedy]


N_NEW = 6
TRUNC = dict(temperature=0.9, top_k=20, top_p=0.8)


@pytest.fixture(scope="module")
def ar_sample(engines):
    """Autoregressive continuations under the truncation, drawn once for the sync and the async comparison."""
    from ssd_amd.sampling_params import SamplingParams
    a, _ = draw(engines["ar"], SamplingParams(max_new_tokens=N_NEW, ignore_eos=True, **TRUNC), 40, 48, N_NEW)
    assert a[:, 1].unique().numel() >= 4, "degenerate test distribution"
    return a


def test_sync_speculation_matches_autoregressive_sampling_under_truncation(engines, ar_sample):
    from ssd_amd.sampling_params import SamplingParams
    t, _ = cfgs()
    s, lens = draw(engines["sync"], SamplingParams(max_new_tokens=N_NEW, ignore_eos=True, **TRUNC), 40, 48, N_NEW)
    print("sync: mean accepted (+recovery)", sum(lens) / len(lens))
    assert min(lens) < K + 1 and max(lens) == K + 1          # rejections and fully accepted rounds: both branches exercised
    assert sum(1 for n in lens if n < K + 1) > 50 and sum(1 for n in lens if n == K + 1) > 50
    for pos in range(1, N_NEW):
        two_sample_ok(ar_sample[:, pos], s[:, pos], t.vocab_size, f"sync, truncated: marginal of generated position {pos}")


def test_async_speculation_matches_autoregressive_sampling_under_truncation(engines, ar_sample):
    from ssd_amd.sampling_params import SamplingParams
    t, _ = cfgs()
    sd = engines["async"]
    before = dict(sd.draft_server.stats)
    s, lens = draw(sd, SamplingParams(max_new_tokens=N_NEW, ignore_eos=True, **TRUNC), 40, 8, N_NEW)
    st = {k: sd.draft_server.stats[k] - before[k] for k in before}
    print("async: mean accepted (+recovery)", sum(lens) / len(lens), "cache hit rate", st["hits"] / max(1, st["requests"]))
    assert 0 < st["hits"] < st["requests"]          # the cached tree branches and the JIT chain both served requests
    assert sum(1 for n in lens if n < K + 1) > 50 and sum(1 for n in lens if n == K + 1) > 50
    for pos in range(1, N_NEW):
        two_sample_ok(ar_sample[:, pos], s[:, pos], t.vocab_size, f"async, truncated: marginal of generated position {pos}")


@pytest.fixture(scope="module")
def same_model(gpu):
    return {"sync": engine("sync", B=8, weights_seed=0, draft_weights_seed=0),
            "async": engine("async", B=8, weights_seed=0, draft_weights_seed=0)}


@pytest.mark.parametrize("mode", ["sync", "async"])
def test_same_model_draft_under_top_p_accepts_nearly_everything(same_model, mode):
    """The existing same-model bar (mean accepted length with recovery above 3.8 of 4): it holds only if q is truncated like p."""
    from ssd_amd.sampling_params import SamplingParams
    eng = same_model[mode]
    lens = []
    for _ in range(4):
        out, m = eng.generate([PROMPT] * 8, SamplingParams(temperature=1.0, top_p=0.5, max_new_tokens=24, ignore_eos=True), use_tqdm=False)
        lens += m["accepted_suffix_lens_with_recovery"]
    print(f"{mode}: mean accepted (+recovery) under top_p=0.5: {sum(lens) / len(lens):.3f} over {len(lens)} rounds")
    assert sum(lens) / len(lens) > 3.8, lens
    assert len({tuple(o["token_ids"]) for o in out}) > 1          # still sampling: rows draw independently


def test_mixed_batch_greedy_stays_greedy_and_first_tokens_come_from_the_kept_set(same_model, monkeypatch):
    from ssd_amd.hip import filter_ops
    from ssd_amd.sampling_params import SamplingParams
    eng = same_model["sync"]
    V = eng.model_runner.cfg.vocab_size
    calls = []
    real = filter_ops.filter_rows

    def spy(logits, ld, T, V_, temps, top_k, top_p, min_p, rows_per_param, kept=None):
        # the target's prefill samples eagerly from the model's own logit buffer: keep the rows as they were before the filter
        if not torch.cuda.is_current_stream_capturing() and logits.data_ptr() == eng.model_runner.model.logits.data_ptr() \
                and rows_per_param == 1 and T == 4:
            calls.append((logits[:T, :V_].clone(), temps[:T].clone(), top_k[:T].clone(), top_p[:T].clone(), min_p[:T].clone()))
        return real(logits, ld, T, V_, temps, top_k, top_p, min_p, rows_per_param, kept)
    monkeypatch.setattr(filter_ops, "filter_rows", spy)
    common = dict(max_new_tokens=16, ignore_eos=True)
    sps = [SamplingParams(temperature=0, **common), SamplingParams(temperature=1.0, **common),
           SamplingParams(temperature=1.2, top_k=3, **common), SamplingParams(temperature=1.5, top_p=0.3, min_p=0.2, **common)]
    greedy, _ = eng.generate([PROMPT], sps[0], use_tqdm=False)
    firsts = []
    for _ in range(12):
        n0 = len(calls)
        mixed, _ = eng.generate([PROMPT] * 4, sps, use_tqdm=False)
        assert mixed[0]["token_ids"] == greedy[0]["token_ids"]
        assert len(calls) > n0, "the prefill of a batch with filtered sequences launched no filter"
        firsts.append((calls[n0], [o["token_ids"][0] for o in mixed]))
    outside_unfiltered = 0.0
    for (lg, temps, ks, ps, ms), toks in firsts:
        lg, temps, ks, ps, ms = lg.float().cpu().numpy(), temps.tolist(), ks.tolist(), ps.tolist(), ms.tolist()
        assert (ks, [round(p, 4) for p in ps], [round(m, 4) for m in ms]) == ([0, 0, 3, 0], [1.0, 1.0, 1.0, 0.3], [0.0, 0.0, 0.0, 0.2])
        for row in (2, 3):
            ref = R.filter_row(lg[row], temps[row], ks[row], ps[row], ms[row])
            assert ref.touched and ref.keep[toks[row]], f"first token {toks[row]} of sequence {row} is outside the kept set"
            e, _ = R.exp_row(lg[row], temps[row])
            outside_unfiltered = max(outside_unfiltered, 1.0 - e[ref.keep].sum() / e.sum())
    # the check has teeth: without the filter a good part of the draws would have fallen outside
    assert outside_unfiltered > 0.2, outside_unfiltered


def test_default_sampling_params_launch_no_filter(same_model):
    from ssd_amd.hip import filter_ops
    from ssd_amd.sampling_params import SamplingParams
    n0 = filter_ops.LAUNCHES
    for mode in ("sync", "async"):
        out, _ = same_model[mode].generate([PROMPT] * 4, SamplingParams(temperature=0.7, max_new_tokens=12, ignore_eos=True), use_tqdm=False)
        assert all(len(o["token_ids"]) == 12 for o in out)
    assert filter_ops.LAUNCHES == n0
    out, _ = same_model["sync"].generate([PROMPT] * 4, SamplingParams(temperature=0.7, top_k=5, max_new_tokens=12, ignore_eos=True), use_tqdm=False)
    assert filter_ops.LAUNCHES > n0          # ... and the counter does count
