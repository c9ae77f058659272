"""SamplingParams(logprobs=N), the parts that need no GPU: the parameter, the per-token records' bookkeeping through Sequence /
Scheduler / Verifier / LLMEngine with hand-made records, the refusal by runners without the kernel, the float64 restatement's own
hand-checked rows, and the C ABI of include/ssd_hip_logprob.h (exports, ctypes table, INTEGRATION.md, a plain-C consumer walking
every entry point's argument validation)."""
import itertools
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.conftest import ROOT
from tests import logprob_ref as R

HEADER = os.path.join(ROOT, "include", "ssd_hip_logprob.h")


# ---------------------------------------------------------------------------------------------------------------------
# public interface
# ---------------------------------------------------------------------------------------------------------------------
def test_sampling_params_logprobs_default_is_off_and_values_are_validated():
    from ssd_amd.sampling_params import SamplingParams
    from ssd_amd.engine.sequence import Sequence
    sp = SamplingParams()
    assert sp.logprobs is None
    # every other default as before
    assert (sp.temperature, sp.draft_temperature, sp.max_new_tokens, sp.ignore_eos) == (1.0, None, 256, False)
    assert (sp.top_k, sp.top_p, sp.min_p) == (0, 1.0, 0.0) and sp.active_filters == [] and sp.active_penalties == []
    assert (sp.repetition_penalty, sp.presence_penalty, sp.frequency_penalty, sp.logit_bias) == (1.0, 0.0, 0.0, None)
    s = Sequence([1, 2, 3], sp)
    assert s.logprobs is None and s.logprob_records == [] and s.recovery_logprob is None and s.completion_logprobs == []
    assert Sequence([1]).logprobs is None
    for n in (0, 1, 20):
        assert SamplingParams(logprobs=n).logprobs == n and Sequence([1, 2], SamplingParams(logprobs=n)).logprobs == n
    for bad in (-1, 21, 1.5, True, False, "3"):
        with pytest.raises(ValueError, match="logprobs"):
            SamplingParams(logprobs=bad)


def test_sampling_selects_its_own_graphs_only_when_asked():
    from ssd_amd.engine.model_runner import GREEDY, ModelRunner, Sampling
    assert GREEDY == Sampling(False, False, False, False) and GREEDY.suffix == ""
    assert [Sampling(*f).suffix for f in ((True,), (True, True), (False, False, True), (True, True, True))] == ["_s", "_sf", "_p", "_sf_p"]
    assert Sampling(lp=True).suffix == "_l" and Sampling(True, True, True, True).suffix == "_sf_p_l"
    assert not Sampling.explicit([0.5], ([1], [1.0], [0.0])).lp          # the draft server's requests never ask
    assert ModelRunner.supports_logprobs


# ---------------------------------------------------------------------------------------------------------------------
# bookkeeping with hand-made records: the record of token t is rec(t), so alignment can be read off the token ids
# ---------------------------------------------------------------------------------------------------------------------
def rec(tok):
    return {"token_id": tok, "logprob": -tok / 100.0, "top_ids": [tok], "top_logprobs": [-tok / 100.0]}


def scheduler(speculate: bool, nblocks: int = 16, eos: int = 5, max_model_len: int = 256, K: int = 3):
    from ssd_amd.engine.scheduler import Scheduler
    from ssd_amd.engine.sequence import Sequence
    Sequence.block_size = 16
    Sequence.counter = itertools.count()
    cfg = SimpleNamespace(max_num_seqs=4, max_num_batched_tokens=256, max_model_len=max_model_len, eos=eos, speculate=speculate,
                          draft_async=False, speculate_k=K, kvcache_block_size=16, num_kvcache_blocks=nblocks, fan_out_list=None)
    return Scheduler(cfg, draft_num_blocks=nblocks if speculate else None)


def new_seq(sch, prompt, **sp):
    from ssd_amd.engine.sequence import Sequence
    from ssd_amd.sampling_params import SamplingParams
    s = Sequence(prompt, SamplingParams(temperature=0.0, **sp))
    sch.add(s)
    return s


def spec_prefill(seqs, toks):
    """What SpecDecodeStep.prefill + Verifier.prefill leave behind."""
    for s, t in zip(seqs, toks):
        s.recovery_token_id, s.recovery_logprob = t, (rec(t) if s.logprobs is not None else None)
        s.num_cached_tokens = s.num_draft_cached_tokens = s.num_prompt_tokens
        s.last_spec_step_accepted_len = -1


def aligned(s):
    P = s.num_request_prompt_tokens
    assert [r["token_id"] for r in s.logprob_records] == s.token_ids[P:], (s.logprob_records, s.token_ids[P:])
    assert [r["token_id"] for r in s.completion_logprobs] == s.completion_token_ids


def test_a_suffix_clipped_at_eos_keeps_records_and_tokens_together():
    sch = scheduler(True, eos=5)
    s = new_seq(sch, [1, 2, 3], logprobs=2, max_new_tokens=50)
    seqs, is_prefill = sch.schedule()
    assert is_prefill and seqs == [s]
    spec_prefill(seqs, [10])
    seqs, is_prefill = sch.schedule()
    assert not is_prefill
    # the round accepted all three draft tokens (11, 5 = EOS, 12); 13 is the new recovery token
    sch.postprocess_speculate(seqs, [[10, 11, 5, 12]], [13], logprobs=[[rec(11), rec(5), rec(12), rec(13)]])
    assert s.is_finished and s.completion_token_ids == [10, 11, 5]
    aligned(s)
    assert s.logprob_records == [rec(10), rec(11), rec(5)]


def test_a_suffix_clipped_at_max_new_tokens_keeps_records_and_tokens_together():
    sch = scheduler(True)
    s = new_seq(sch, [1, 2, 3], logprobs=0, max_new_tokens=6, ignore_eos=True)
    other = new_seq(sch, [4, 2], max_new_tokens=6, ignore_eos=True)          # did not ask: no records, whatever the runner hands up
    seqs, _ = sch.schedule()
    spec_prefill(seqs, [10, 30])
    seqs, _ = sch.schedule()
    sch.postprocess_speculate(seqs, [[10, 11, 12, 13], [30]], [14, 31], logprobs=[[rec(11), rec(12), rec(13), rec(14)], None])
    assert s.completion_token_ids == [10, 11, 12, 13] and s.recovery_logprob == rec(14) and not s.is_finished
    aligned(s)
    seqs, _ = sch.schedule()
    sch.postprocess_speculate(seqs, [[14, 15, 16], [31, 32]], [17, 33], logprobs=[[rec(15), rec(16), rec(17)], None])
    assert s.is_finished and s.completion_token_ids == [10, 11, 12, 13, 14, 15]          # 16 fell to max_new_tokens, with its record
    aligned(s)
    assert other.logprob_records == [] and other.recovery_logprob is None and other.completion_token_ids == [30, 31, 32]


@pytest.mark.parametrize("speculate", [False, True])
def test_a_preempted_and_reprefilled_sequence_neither_loses_nor_doubles_a_record(speculate):
    sch = scheduler(speculate)
    s = new_seq(sch, [1, 2, 3], logprobs=1, max_new_tokens=50, ignore_eos=True)
    seqs, is_prefill = sch.schedule()
    assert is_prefill
    if speculate:
        spec_prefill(seqs, [10])
        seqs, _ = sch.schedule()
        sch.postprocess_speculate(seqs, [[10, 11]], [12], logprobs=[[rec(11), rec(12)]])
        assert s.recovery_logprob == rec(12)
    else:
        sch.postprocess(seqs, [10], True, logprobs=[rec(10)])
        seqs, _ = sch.schedule()
        sch.postprocess(seqs, [11], False, logprobs=[rec(11)])
    aligned(s)
    sch.preempt(sch.running.pop())
    assert s.num_prompt_tokens == 5 and s.num_request_prompt_tokens == 3 and s.completion_token_ids == []
    assert s.recovery_logprob is None                  # the pending recovery token went with the preemption, and so did its record
    assert s.logprob_records == [rec(10), rec(11)] and s.completion_logprobs == []
    seqs, is_prefill = sch.schedule()
    assert is_prefill and seqs == [s]
    if speculate:
        spec_prefill(seqs, [20])                       # the re-prefill's token and record
        seqs, _ = sch.schedule()
        sch.postprocess_speculate(seqs, [[20, 21, 22]], [23], logprobs=[[rec(21), rec(22), rec(23)]])
        assert s.completion_token_ids == [20, 21, 22]
    else:
        sch.postprocess(seqs, [20], True, logprobs=[rec(20)])
        seqs, _ = sch.schedule()
        sch.postprocess(seqs, [21], False, logprobs=[rec(21)])
        assert s.completion_token_ids == [20, 21]
    aligned(s)
    assert s.token_ids[:5] == [1, 2, 3, 10, 11] and s.logprob_records[:2] == [rec(10), rec(11)]


class StubRunner:
    """What Verifier.prefill needs of a runner: run -> tokens, the records beside them in last_logprobs."""
    def __init__(self):
        self.next = []

    def call(self, method, seqs, is_prefill):
        assert method == "run" and is_prefill
        toks = [self.next.pop(0) for _ in seqs]
        self.last_logprobs = [rec(t) if s.logprobs is not None else None for s, t in zip(seqs, toks)]
        return toks


def test_the_pinned_first_token_keeps_its_record_through_a_reprefill():
    from ssd_amd.engine.verifier import Verifier
    sch = scheduler(True)
    s = new_seq(sch, [1, 2, 3], logprobs=3, max_new_tokens=50, ignore_eos=True)
    quiet = new_seq(sch, [1, 2], max_new_tokens=50, ignore_eos=True)
    runner = StubRunner()
    ver = Verifier(3, None, runner)
    seqs, _ = sch.schedule()
    runner.next = [10, 40]
    out = ver.prefill(seqs)
    assert out.recovery_tokens == [10, 40] and s.recovery_logprob == rec(10) and quiet.recovery_logprob is None
    s.first_token_streamed = 10                        # LLMEngine.generate handed it to the stream
    while sch.running:
        sch.preempt(sch.running.pop())
    assert s.recovery_token_id is None and s.recovery_logprob == rec(10)
    seqs, is_prefill = sch.schedule()
    assert is_prefill and s in seqs
    runner.next = [77, 78]                             # the re-prefill flips the near-tie: the pinned token and ITS record stay
    ver.prefill(seqs)
    assert s.recovery_token_id == 10 and s.recovery_logprob == rec(10)
    for q in seqs:
        q.num_cached_tokens = q.num_draft_cached_tokens = q.num_prompt_tokens
        q.first_token_streamed = None                  # (the speculator's append_token of the recovery token clears the pin)
    seqs, _ = sch.schedule()
    sch.postprocess_speculate(seqs, [[q.recovery_token_id, 11] for q in seqs], [12, 12], logprobs=[[rec(11), rec(12)]] * 2)
    aligned(s)
    # without the pin (preempted after the first round) the fresh token and its record are taken
    sch.preempt(s)
    sch.running.remove(s)
    assert s.recovery_logprob is None
    seqs, _ = sch.schedule()
    runner.next = [55]
    ver.prefill(seqs)
    assert (s.recovery_token_id, s.recovery_logprob) == (55, rec(55))


class FakeSpecStep:
    """A speculation step with hand-made tokens and records: every round accepts two draft tokens."""
    def __init__(self, scheduler):
        self.scheduler, self.tok = scheduler, itertools.count(100)

    def prefill(self, seqs):
        spec_prefill(seqs, [next(self.tok) for _ in seqs])
        return sum(len(s) for s in seqs)

    def decode(self, seqs):
        sfx, nxt, lps = [], [], []
        for s in seqs:
            a, b, r = next(self.tok), next(self.tok), next(self.tok)
            sfx.append([s.recovery_token_id, a, b])
            nxt.append(r)
            lps.append([rec(a), rec(b), rec(r)] if s.logprobs is not None else None)
        self.scheduler.postprocess_speculate(seqs, sfx, nxt, logprobs=lps)
        return sum(len(x) for x in sfx)


def oracle_engines(golden, **kw):
    from oracle.runner import oracle_runner_factory
    from ssd_amd.engine.llm_engine import LLMEngine
    from tests.test_engine_cpu import mcfg, weights, COMMON
    g = golden("engine_golden")
    wt, wd = weights(g, "t."), weights(g, "d.")
    common = dict(COMMON, **kw)
    ar = LLMEngine("tiny", hf_config=mcfg(g, "t_"), runner_factory=oracle_runner_factory(wt), **common)
    sd = LLMEngine("tiny", hf_config=mcfg(g, "t_"), draft="tiny-draft", draft_hf_config=mcfg(g, "d_"), speculate=True, speculate_k=3,
                   runner_factory=oracle_runner_factory(wt, wd), **common)
    return ar, sd


def test_generate_returns_records_and_the_capped_path_carries_the_first_tokens_record(golden, monkeypatch):
    from ssd_amd.sampling_params import SamplingParams
    _, sd = oracle_engines(golden, max_model_len=32)
    sd.model_runner.supports_logprobs = True           # (this test drives the engine with a hand-made step, not with the runner)
    monkeypatch.setattr(sd, "create_inference_step", lambda config: FakeSpecStep(sd.scheduler))
    long_prompt = list(range(1, 30))                   # 29 + (K + 1) > 32: capped before its first round, after the first token streamed
    streamed = {}
    sps = [SamplingParams(temperature=0, max_new_tokens=5, ignore_eos=True, logprobs=1),
           SamplingParams(temperature=0, max_new_tokens=5, ignore_eos=True),
           SamplingParams(temperature=0, max_new_tokens=5, ignore_eos=True, logprobs=0)]
    out, _ = sd.generate([[1, 2, 3], [4, 5, 6], long_prompt], sps, use_tqdm=False,
                         stream_callback=lambda sid, toks: streamed.setdefault(sid, []).extend(toks))
    asked, quiet, capped = out
    assert set(quiet) == {"text", "token_ids", "finish_reason"}          # exactly today's dict
    assert len(asked["token_ids"]) == 5 and [r["token_id"] for r in asked["logprobs"]] == asked["token_ids"]
    assert asked["logprobs"] == [rec(t) for t in asked["token_ids"]]
    assert asked["cumulative_logprob"] == pytest.approx(sum(-t / 100.0 for t in asked["token_ids"]))
    assert capped["finish_reason"] == "max_model_len" and len(capped["token_ids"]) == 1
    assert capped["logprobs"] == [rec(capped["token_ids"][0])] and capped["cumulative_logprob"] == capped["logprobs"][0]["logprob"]
    assert sorted(streamed.values(), key=len)[0] == capped["token_ids"]          # what the stream already delivered
    # a second generate starts clean
    out2, _ = sd.generate([[1, 2, 3]], sps[1], use_tqdm=False)
    assert set(out2[0]) == {"text", "token_ids", "finish_reason"}


def test_runners_without_the_kernel_refuse_logprobs_by_name(golden):
    from ssd_amd.sampling_params import SamplingParams
    for eng in oracle_engines(golden):
        assert not getattr(eng.model_runner, "supports_logprobs", False)
        for n in (0, 5):
            with pytest.raises(ValueError, match="logprobs"):
                eng.add_request([1, 2, 3], SamplingParams(temperature=0, logprobs=n))
        assert eng.is_finished()                       # nothing was queued by the refused requests
        eng.add_request([1, 2, 3], SamplingParams(temperature=0, max_new_tokens=2, ignore_eos=True))          # logprobs=None is taken
        assert not eng.is_finished()


def test_a_tensor_parallel_target_refuses_logprobs_by_name(golden):
    from ssd_amd.sampling_params import SamplingParams
    ar, _ = oracle_engines(golden)
    ar.model_runner.supports_logprobs, ar.model_runner.tp_size = True, 2
    with pytest.raises(ValueError, match="logprobs.*tensor-parallel"):
        ar.add_request([1, 2, 3], SamplingParams(temperature=0, logprobs=0))
    assert ar.is_finished()
    ar.model_runner.tp_size = 1
    ar.add_request([1, 2, 3], SamplingParams(temperature=0, logprobs=0))
    assert not ar.is_finished()


# ---------------------------------------------------------------------------------------------------------------------
# the reference itself, on rows small enough to check by hand
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_on_hand_made_rows():
    x = np.array([0.0, -1, -2, -3, -4, -5, -6, -6]) * np.log(2.0)          # probabilities 1/2, 1/4, ... 1/128, 1/128
    r = R.logprob_row(x, 3)
    assert abs(r.lse - np.log(2.0)) < 1e-12             # the weights 1, 1/2, ... sum to 2
    assert np.allclose(r.logprob, np.log([1 / 2, 1 / 4, 1 / 8, 1 / 16, 1 / 32, 1 / 64, 1 / 128, 1 / 128]), atol=1e-12)
    assert r.top_id == [0, 1, 2] and np.allclose(r.top_val, np.log([1 / 2, 1 / 4, 1 / 8]))
    assert R.logprob_row(x, 0).top_id == [] and R.logprob_row(x, 0).top_val == []
    # ties keep index order, also between -0.0 and +0.0; NaN is not comparable; n_top above the comparable entries pads with -1 / -inf
    y = np.array([1.0, np.nan, 0.0, -0.0, -np.inf, 3.0, 3.0, 2.0])
    r = R.logprob_row(y, 8)
    assert r.top_id == [5, 6, 7, 0, 2, 3, 4, -1] and r.top_val[-1] == -np.inf and r.top_val[-2] == -np.inf
    want = np.log(2 * np.exp(3.0) + np.exp(2.0) + np.exp(1.0) + 2.0)
    assert abs(r.lse - want) < 1e-12 and np.isnan(r.logprob[1]) and r.top_val[0] == r.top_val[1] == 3.0 - r.lse
    assert R.pick(y, 5, r.lse) == 3.0 - r.lse and np.isnan(R.pick(y, -1, r.lse)) and np.isnan(R.pick(y, 8, r.lse))
    # a maximum that is not finite: all mass on its class
    z = np.array([np.inf, 1.0, np.inf, np.nan, -np.inf, np.inf])
    r = R.logprob_row(z, 4)
    assert r.lse == np.inf and r.top_id == [0, 2, 5, 1] and np.allclose(r.top_val[:3], -np.log(3.0)) and r.top_val[3] == -np.inf
    r = R.logprob_row(np.array([2.0, np.inf]), 2)
    assert r.lse == np.inf and r.top_id == [1, 0] and r.top_val == [0.0, -np.inf]
    r = R.logprob_row(np.array([-np.inf, np.nan, -np.inf]), 3)
    assert r.lse == -np.inf and r.top_id == [0, 2, -1] and np.allclose(r.top_val[:2], -np.log(2.0))
    # nothing comparable
    r = R.logprob_row(np.full(4, np.nan), 2)
    assert np.isnan(r.lse) and r.top_id == [-1, -1] and r.top_val == [-np.inf, -np.inf]
    # the verify rows' tokens
    assert R.verify_tokens([9, 1, 2, 3], 0, 7) == [7, None, None, None]
    assert R.verify_tokens([9, 1, 2, 3], 2, 7) == [1, 2, 7, None]
    assert R.verify_tokens([9, 1, 2, 3], 3, 7) == [1, 2, 3, 7]


def test_reference_matches_log_softmax_on_random_rows():
    g = torch.Generator().manual_seed(5)
    for V in (1, 7, 33, 1000, 4097):
        x = ((torch.rand(V, generator=g, dtype=torch.float64) - 0.5) * 60).to(torch.bfloat16).to(torch.float64)
        want = torch.log_softmax(x, dim=-1)
        r = R.logprob_row(x.numpy(), min(5, V))
        assert np.abs(r.logprob - want.numpy()).max() < 1e-12
        assert abs(r.lse - float(torch.logsumexp(x, dim=-1))) < 1e-12
        vals, _ = torch.sort(want, descending=True, stable=True)
        assert np.allclose(r.top_val, vals[:min(5, V)].numpy(), atol=1e-12)
        assert all(x[i] == x[j] and i < j or x[i] > x[j] for i, j in zip(r.top_id, r.top_id[1:]))


# ---------------------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------------------
def _built_lib():
    from ssd_amd.hip.lib import build_library, lib_path
    if not os.path.exists(lib_path()):
        build_library()
    return lib_path()


def logprob_header_symbols():
    return sorted(set(re.findall(r"^int\s+(ssd_\w+)\s*\(", open(HEADER).read(), flags=re.M)))


def test_logprob_header_symbols_exported_bound_and_documented():
    from ssd_amd.hip.lib import SIGNATURES, ABI_VERSION
    from ssd_amd.hip import logprob_ops
    from ssd_amd.sampling_params import MAX_LOGPROBS
    _built_lib()
    lib = logprob_ops.load_logprob_library()
    syms = logprob_header_symbols()
    assert syms == ["ssd_logprob_pick", "ssd_logprob_pick_verify", "ssd_logprob_rows", "ssd_logprob_rows_ws_bytes"]
    assert sorted(logprob_ops.LOGPROB_SIGNATURES) == syms
    assert not set(syms) & set(SIGNATURES)             # lib.SIGNATURES stays exactly ssd_hip.h + ssd_hip_tune.h
    assert lib.ssd_abi_version() == ABI_VERSION == 3   # additive header: the ABI version does not move
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    head = open(HEADER).read()
    for s in syms:
        assert hasattr(lib, s), f"{s} not exported"
        assert f"`{s}(" in doc, f"{s} has no line in INTEGRATION.md"
        decl = re.search(r"^int\s+" + s + r"\s*\(([^;]*)\);", head, flags=re.M | re.S).group(1)
        assert len(logprob_ops.LOGPROB_SIGNATURES[s]) == len(decl.split(",")), s
    assert int(re.search(r"#define SSD_LOGPROB_MAX_N (\d+)", head).group(1)) == logprob_ops.MAX_N == R.MAX_N == MAX_LOGPROBS == 20
    assert int(re.search(r"#define SSD_LOGPROB_MAX_V (\d+)", head).group(1)) == logprob_ops.MAX_V >= 196608
    assert "raw" in head.lower() and "before penalties" in head          # which distribution: stated where the semantics live
    common = open(os.path.join(ROOT, "ssd_amd", "csrc", "common.h")).read()
    assert '#include "ssd_hip_logprob.h"' in common
    mk = open(os.path.join(ROOT, "ssd_amd", "csrc", "Makefile")).read()
    assert "../../include/ssd_hip_logprob.h" in mk and "logprob.hip" in mk
    assert logprob_ops.LAUNCHES == 0                   # loading and binding launch nothing
    # the workspace query answers on the host
    one = logprob_ops.logprob_rows_ws_bytes(1, 4096)
    assert one > 0 and logprob_ops.logprob_rows_ws_bytes(3, 4097) == 6 * one and logprob_ops.LAUNCHES == 0


def test_c_consumer_walks_every_logprob_validation_path(tmp_path):
    lib = _built_lib()
    src = os.path.join(ROOT, "tests", "logprob_abi_consumer.c")
    body = open(src).read()
    for s in logprob_header_symbols():
        assert f"{s}(" in body, s
    for what in ("zero T", "zero V", "zero rows_per_param", "ld below V", "above SSD_LOGPROB_MAX_V", "raw_ld below V", "null rows",
                 "null n_top", "null lse", "null top_val alone", "null top_id alone", "null ws", "null tokens", "null out", "null ids",
                 "null accept", "null recovery", "workspace query"):
        assert what in body, what
    exe = str(tmp_path / "logprob_abi_consumer")
    libdir = os.path.dirname(lib)
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-L", libdir, "-lssdhip",
                    f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "0 failures" in run.stdout
