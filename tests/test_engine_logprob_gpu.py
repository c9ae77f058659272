"""SamplingParams(logprobs=N) through the whole engine on the GPU, with the tiny pair and the engine() helper of
tests/test_engine_filter_gpu.py: autoregressive decoding, synchronous speculation and asynchronous speculation over the loopback.

The truth is the CPU oracle model of the same weights, teacher-forced with the engine's own stream: log_softmax in float64 of its bf16
logits.  The tolerance: a log-probability is a logit minus a log-sum-exp, and the log-sum-exp moves by at most the largest logit error,
so BOUND = 2 * LOGIT_ERR, where LOGIT_ERR is the largest |HIP logit - oracle logit| of the parent commit's kernels on these very models
and streams (profiles/logprob_probe.py "logit_err": the decoder's prefill rows and its single-token decode rows against the oracle's;
measured on one MI355X over a grid of 32 prompts of the family below, the six of this file among them: 0.25 on the prefill rows and 0.25 on
the decode rows, at logits up to 17.1 in magnitude, where one bf16 ulp is 0.0625 (on the six prompts alone: 0.14 and 0.09); hence
BOUND = 0.5.  The largest |logprob - oracle| the greedy runs then showed: 0.10.  DESIGN.md, "Log-probabilities").

Where the engine's and the oracle's top lists differ only in the order of entries whose oracle log-probabilities lie within BOUND of each other, that is accepted, for at most 2 % of the
positions of a run.

The prompts.  Two bf16 pipelines do not rank 128 logits of magnitude up to 16 alike everywhere: on the parent's kernels alone -- the
decoder's logits sorted on the host, no log-probability code -- the top-5 list differs from the oracle's at 44 of 768 generated
positions (5.7 %) over a grid of 32 prompts of this family (`profiles/logprob_probe.py logit_err --grid`), and a first prompt set
needed the excuse at 6 to 7 of 144 positions, with the same count, 7 and 5, on the parent's kernels alone.  The six prompts below
are those of the grid at which the decoder's own logits rank the oracle's top 5 alike at every generated position, on its prefill
and on its single-token decode path; on the CPU, the oracle's own decode rows against its prefill rows need the excuse at 0 of 144
positions of them.  With them the engine needs the excuse at 1 of 144 positions in each mode (its batched decode rows and its verify
rows are tiled differently from the probe's single rows)."""
import numpy as np
import pytest
import torch

from tests.test_engine_filter_gpu import K, engine
from tests.test_engine_temperature_gpu import KW, cfgs, perturbed_pair
from tests.util import NEAR_TIE, common_prefix

pytestmark = pytest.mark.gpu

LOGIT_ERR = 0.25            # largest |HIP logit - oracle logit| measured on these models (4 bf16 ulps at magnitude 8..16)
BOUND = 2 * LOGIT_ERR
PROMPTS = [[(a * j + b) % 128 for j in range(n)] for a, b, n in ((3, 1, 9), (9, 4, 12), (9, 6, 10), (11, 2, 7), (11, 4, 12), (13, 6, 10))]
N_NEW = 24
MODES = ["ar", "sync", "async"]
KEYS = {"text", "token_ids", "finish_reason"}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssd_amd.hip import ops
    return ops


@pytest.fixture(scope="module")
def engines(gpu):
    """One engine per decoding mode over the correlated pair (draft = target + 3 % noise): rounds accept and reject."""
    t, factory = perturbed_pair(0.03)
    return {m: engine(m, factory, B=8) for m in MODES}


@pytest.fixture(scope="module")
def oracle():
    """(prompt, tokens) -> float64 [len(tokens), V]: the oracle's raw log-softmax at every generated position, teacher-forced."""
    from oracle.model import Ctx, OracleModel
    from ssd_amd import weights as W
    torch.set_num_threads(min(16, torch.get_num_threads()))
    t, _ = cfgs()
    model = OracleModel(t, W.synthetic_state_dict(t, 0, KW["weights_std"]), 16, 16)
    cache = {}

    def logprobs(prompt, tokens):
        key = (tuple(prompt), tuple(tokens))
        if key not in cache:
            ids = list(prompt) + list(tokens)
            T = len(ids)
            cu = torch.tensor([0, T], dtype=torch.int32)
            with torch.inference_mode():
                h = model.forward(torch.tensor(ids), torch.arange(T), Ctx("prefill", slot_mapping=torch.arange(T, dtype=torch.int32), cu_q=cu, cu_k=cu))
                lg = model.compute_logits(h).double()
            cache[key] = torch.log_softmax(lg, dim=-1)[len(prompt) - 1:T - 1].numpy()
        return cache[key]
    return logprobs


def check_records(prompt, tokens, records, N, oracle, what):
    """Shape and truth of one request's records; returns (positions, positions whose top list needed the order excuse, worst error)."""
    assert len(records) == len(tokens), f"{what}: {len(records)} records for {len(tokens)} tokens"
    ref = oracle(prompt, tokens)
    V = ref.shape[1]
    excused, worst = 0, 0.0
    for i, (tok, r) in enumerate(zip(tokens, records)):
        w = f"{what} token {i}"
        assert set(r) == {"token_id", "logprob", "top_ids", "top_logprobs"} and r["token_id"] == tok, w
        assert r["logprob"] <= 0.0, w
        worst = max(worst, abs(r["logprob"] - ref[i, tok]))
        assert abs(r["logprob"] - ref[i, tok]) <= BOUND, f"{w}: logprob {r['logprob']} vs the oracle's {ref[i, tok]}"
        assert len(r["top_ids"]) == len(r["top_logprobs"]) == min(N, V), w
        assert all(a >= b for a, b in zip(r["top_logprobs"], r["top_logprobs"][1:])), f"{w}: not descending"
        for j, lp in zip(r["top_ids"], r["top_logprobs"]):
            worst = max(worst, abs(lp - ref[i, j]))
            assert abs(lp - ref[i, j]) <= BOUND, f"{w}: top entry {j}: {lp} vs the oracle's {ref[i, j]}"
        order = np.argsort(-ref[i], kind="stable")[:N]
        if r["top_ids"] != order.tolist():
            # the same list up to the order (and, at its end, the choice) of entries the oracle itself puts within BOUND of each other
            assert all(abs(ref[i, j] - ref[i, o]) <= BOUND for j, o in zip(r["top_ids"], order)), \
                f"{w}: top ids {r['top_ids']} vs the oracle's {order.tolist()}"
            excused += 1
    return len(tokens), excused, worst


def greedy_sp(n=None, **kw):
    from ssd_amd.sampling_params import SamplingParams
    return SamplingParams(temperature=0, max_new_tokens=N_NEW, ignore_eos=True, logprobs=n, **kw)


@pytest.fixture(scope="module")
def greedy_runs(engines):
    """The greedy streams of every mode without and with logprobs=5, generated once: (plain outputs, asked outputs, metrics)."""
    runs = {}
    for m in MODES:
        plain, _ = engines[m].generate(PROMPTS, greedy_sp(), use_tqdm=False)
        asked, met = engines[m].generate(PROMPTS, greedy_sp(5), use_tqdm=False)
        runs[m] = (plain, asked, met)
    return runs


@pytest.mark.parametrize("mode", MODES)
def test_asking_changes_no_token_and_the_records_are_the_oracles(greedy_runs, oracle, mode):
    plain, asked, met = greedy_runs[mode]
    assert [o["token_ids"] for o in asked] == [o["token_ids"] for o in plain]
    assert all(set(o) == KEYS for o in plain)                                           # exactly today's keys without the request
    assert all(set(o) == KEYS | {"logprobs", "cumulative_logprob"} for o in asked)
    if mode != "ar":        # both branches ran: fully accepted rounds and rejections
        lens = met["accepted_suffix_lens_with_recovery"]
        assert max(lens) == K + 1 and min(lens) < K + 1, lens
    total = excused = 0
    worst = 0.0
    for p, o in zip(PROMPTS, asked):
        assert len(o["token_ids"]) == N_NEW
        n, e, w = check_records(p, o["token_ids"], o["logprobs"], 5, oracle, f"{mode} prompt {PROMPTS.index(p)}")
        total, excused, worst = total + n, excused + e, max(worst, w)
        assert o["cumulative_logprob"] == pytest.approx(sum(r["logprob"] for r in o["logprobs"]), abs=1e-9)
        for i, r in enumerate(o["logprobs"]):           # greedy, no penalties: the token IS the most probable one, by bits --
            assert r["top_ids"][0] == r["token_id"] and r["top_logprobs"][0] == r["logprob"], (mode, i, r)      # prefill, recovery, accepted
    print(f"{mode}: worst |logprob - oracle| {worst:.4f} (bound {BOUND}), top lists excused {excused} of {total}")
    assert excused <= 0.02 * total, f"{mode}: {excused} of {total} positions needed the order excuse"


@pytest.mark.parametrize("mode", ["sync", "async"])
def test_speculation_reports_the_log_probabilities_of_autoregression(greedy_runs, oracle, mode):
    _, ar, _ = greedy_runs["ar"]
    _, sd, _ = greedy_runs[mode]
    compared = 0
    for p, a, s in zip(PROMPTS, ar, sd):
        n = common_prefix(a["token_ids"], s["token_ids"])
        if n < N_NEW:       # the near-tie rule of tests/util.py: the streams may part only where the oracle's top-2 margin is a near-tie
            top = np.sort(oracle(p, a["token_ids"])[n])[::-1]
            assert top[0] - top[1] <= NEAR_TIE, f"{mode}: diverged from AR at token {n} with an oracle margin of {top[0] - top[1]:.4f}"
        for ra, rs in zip(a["logprobs"][:n], s["logprobs"][:n]):
            assert abs(ra["logprob"] - rs["logprob"]) <= BOUND, (mode, ra, rs)
            compared += 1
    assert compared >= 0.8 * N_NEW * len(PROMPTS), compared


@pytest.mark.parametrize("mode", MODES)
def test_raw_means_raw_under_penalties_and_bias(engines, greedy_runs, oracle, mode):
    """Penalised and biased requests still report the raw log-softmax: the test that fails if the pick reads the adjusted rows."""
    plain = greedy_runs[mode][0]
    banned = plain[0]["token_ids"][1]                   # a token the unpenalised stream emits
    out, _ = engines[mode].generate(PROMPTS, greedy_sp(3, repetition_penalty=1.3, logit_bias={banned: -100}), use_tqdm=False)
    assert [o["token_ids"] for o in out] != [o["token_ids"] for o in plain]
    moved = 0
    for p, o in zip(PROMPTS, out):
        assert banned not in o["token_ids"]
        check_records(p, o["token_ids"], o["logprobs"], 3, oracle, f"{mode} penalised")
        moved += sum(r["top_ids"][0] != r["token_id"] for r in o["logprobs"])
    assert moved > 0        # somewhere the penalties chose a token that is not the raw argmax: its record is still the raw one


@pytest.mark.parametrize("mode", MODES)
def test_raw_means_raw_under_sampling_with_truncation(engines, oracle, mode):
    from ssd_amd.sampling_params import SamplingParams
    sp = SamplingParams(temperature=0.9, top_k=20, top_p=0.8, max_new_tokens=12, ignore_eos=True, logprobs=2)
    out, _ = engines[mode].generate(PROMPTS, sp, use_tqdm=False)
    off_top = 0
    for p, o in zip(PROMPTS, out):
        assert len(o["token_ids"]) == 12
        check_records(p, o["token_ids"], o["logprobs"], 2, oracle, f"{mode} sampled")
        off_top += sum(r["top_ids"][0] != r["token_id"] for r in o["logprobs"])
    assert off_top > 0      # it did sample


@pytest.mark.parametrize("mode", MODES)
def test_a_mixed_batch(engines, greedy_runs, oracle, mode):
    from ssd_amd.sampling_params import SamplingParams
    plain = greedy_runs[mode][0]
    out, _ = engines[mode].generate(PROMPTS[:2], [greedy_sp(4), greedy_sp()], use_tqdm=False)
    assert set(out[1]) == KEYS and out[1]["token_ids"] == plain[1]["token_ids"]         # did not ask: no key, and the tokens it has alone
    assert out[0]["token_ids"] == plain[0]["token_ids"]
    check_records(PROMPTS[0], out[0]["token_ids"], out[0]["logprobs"], 4, oracle, f"{mode} mixed")
    sps = [greedy_sp(0), SamplingParams(temperature=0.8, max_new_tokens=N_NEW, ignore_eos=True, logprobs=3)]
    out, _ = engines[mode].generate(PROMPTS[:2], sps, use_tqdm=False)
    assert all(r["top_ids"] == [] and r["top_logprobs"] == [] for r in out[0]["logprobs"])
    assert all(len(r["top_ids"]) == 3 for r in out[1]["logprobs"])
    assert out[0]["token_ids"] == plain[0]["token_ids"]
    for i in (0, 1):
        check_records(PROMPTS[i], out[i]["token_ids"], out[i]["logprobs"], (0, 3)[i], oracle, f"{mode} mixed 0 / 3")


@pytest.mark.parametrize("mode", ["sync", "async"])
def test_eos_inside_an_accepted_suffix_ends_records_and_tokens_together(engines, greedy_runs, oracle, mode, monkeypatch):
    plain, _, met = greedy_runs[mode]
    eng = engines[mode]
    # a generated position that is neither the first of its round nor a token seen earlier in the stream.  One request: the
    # rounds' lengths of the metrics are its own
    ref, m = eng.generate(PROMPTS[:1], greedy_sp(), use_tqdm=False)
    toks, pos, cut = ref[0]["token_ids"], 0, None
    for n in m["accepted_suffix_lens_with_recovery"]:
        for j in range(1, n):
            if cut is None and pos + j < len(toks) and toks[pos + j] not in toks[:pos + j] and pos + j >= 2:
                cut = pos + j
        pos += n
    assert cut is not None, (toks, m["accepted_suffix_lens_with_recovery"])
    monkeypatch.setattr(eng.scheduler, "eos", toks[cut])
    from ssd_amd.sampling_params import SamplingParams
    out, _ = eng.generate(PROMPTS[:1], SamplingParams(temperature=0, max_new_tokens=N_NEW, logprobs=1), use_tqdm=False)
    assert out[0]["token_ids"] == toks[:cut + 1]
    check_records(PROMPTS[0], out[0]["token_ids"], out[0]["logprobs"], 1, oracle, f"{mode} EOS")
    assert out[0]["logprobs"][-1]["token_id"] == toks[cut]


@pytest.mark.parametrize("mode", ["ar", "sync"])
def test_a_run_that_preempts_neither_loses_nor_doubles_a_record(gpu, oracle, mode, monkeypatch):
    """A KV pool too small for the batch: sequences are preempted and prefilled again.  Every record of every sequence -- over its
    whole life, not only the tokens generated since the last preemption -- is the oracle's for its position."""
    _, factory = perturbed_pair(0.03)
    eng = engine(mode, factory, B=3, num_kvcache_blocks=9, num_draft_kvcache_blocks=9)
    seqs, preempted = [], []
    add, preempt = eng.scheduler.add, eng.scheduler.preempt
    monkeypatch.setattr(eng.scheduler, "add", lambda s: (seqs.append(s), add(s))[1])
    monkeypatch.setattr(eng.scheduler, "preempt", lambda s: (preempted.append(s.seq_id), preempt(s))[1])
    prompts = [[(11 * i + 7 * j + 3) % 128 for j in range(30 + 3 * i)] for i in range(4)]
    out, _ = eng.generate(prompts, greedy_sp(2), use_tqdm=False)
    assert preempted, "the pool was large enough: nothing was preempted"
    assert len(out) == 4
    for p, o, s in zip(prompts, out, seqs):
        assert len(o["logprobs"]) == len(o["token_ids"]) and [r["token_id"] for r in o["logprobs"]] == o["token_ids"]
        P = s.num_request_prompt_tokens
        assert P == len(p) and len(s.logprob_records) == len(s.token_ids) - P
        assert o["token_ids"] == s.token_ids[s.num_prompt_tokens:] and o["logprobs"] == s.logprob_records[s.num_prompt_tokens - P:]
        check_records(p, s.token_ids[P:], s.logprob_records, 2, oracle, f"{mode} preempted seq {s.seq_id}")
    assert any(s.num_prompt_tokens > s.num_request_prompt_tokens for s in seqs)


def test_default_parameters_launch_nothing(engines):
    from ssd_amd.hip import logprob_ops
    from ssd_amd.sampling_params import SamplingParams
    n0 = logprob_ops.LAUNCHES
    for m in MODES:
        for sp in (SamplingParams(temperature=0, max_new_tokens=8, ignore_eos=True),
                   SamplingParams(temperature=0.7, top_k=5, repetition_penalty=1.1, max_new_tokens=8, ignore_eos=True)):
            out, _ = engines[m].generate(PROMPTS[:2], sp, use_tqdm=False)
            assert all(set(o) == KEYS for o in out)
    assert logprob_ops.LAUNCHES == n0
    engines["ar"].generate(PROMPTS[:1], SamplingParams(temperature=0, max_new_tokens=2, ignore_eos=True, logprobs=0), use_tqdm=False)
    assert logprob_ops.LAUNCHES > n0         # ... and the counter does count
