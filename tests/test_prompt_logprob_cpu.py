"""SamplingParams(prompt_logprobs=N), the parts that need no GPU: the parameter, the float64 restatement of the rank, the C ABI of
include/ssd_hip_prompt_logprob.h (exports, ctypes table, INTEGRATION.md, a plain-C consumer), the block manager's "no hit, but leave
the hashes" rule, the records' bookkeeping through Sequence / Scheduler / the steps / LLMEngine with hand-made records, the refusal by
runners without the kernel, and a default run that launches nothing of it."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests.conftest import ROOT
from tests import logprob_ref as R
from tests import prompt_logprob_ref as PR
from tests.test_logprob_cpu import _built_lib, new_seq, oracle_engines, scheduler

HEADER = os.path.join(ROOT, "include", "ssd_hip_prompt_logprob.h")


# ---------------------------------------------------------------------------------------------------------------------
# public interface
# ---------------------------------------------------------------------------------------------------------------------
def test_sampling_params_prompt_logprobs_default_is_off_and_values_are_validated():
    from ssd_amd.sampling_params import SamplingParams
    from ssd_amd.engine.sequence import Sequence
    sp = SamplingParams()
    assert sp.prompt_logprobs is None and sp.logprobs is None
    s = Sequence([1, 2, 3], sp)
    assert s.prompt_logprobs is None and s.prompt_logprob_records is None and not s.needs_prompt_logprobs
    assert not Sequence([1]).needs_prompt_logprobs
    for n in (0, 1, 20):
        assert SamplingParams(prompt_logprobs=n).prompt_logprobs == n
        q = Sequence([1, 2], SamplingParams(prompt_logprobs=n))
        assert q.prompt_logprobs == n and q.needs_prompt_logprobs and q.logprobs is None       # the two parameters are independent
    for bad in (-1, 21, 1.5, True, False, "3"):
        with pytest.raises(ValueError, match="prompt_logprobs"):
            SamplingParams(prompt_logprobs=bad)
    from ssd_amd.engine.model_runner import ModelRunner
    assert ModelRunner.supports_prompt_logprobs and ModelRunner.PROMPT_LOGPROB_ROWS in (128, 256, 512)
    assert "prompt_logprobs=N" in __import__("ssd_amd.sampling_params").sampling_params.__doc__


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_rank_on_hand_made_rows():
    nan, inf = np.nan, np.inf
    y = np.array([1.0, nan, 0.0, -0.0, -inf, 3.0, 3.0, 2.0])
    assert [PR.rank(y, t) for t in range(8)] == [4, 0, 6, 6, 7, 2, 2, 3]     # tied maxima both 2; the zeros are one value; -inf: all 7
    assert PR.rank(y, -1) == 0 and PR.rank(y, 8) == 0
    assert PR.rank(np.array([5.0, 1.0]), 0) == 1 and PR.rank(np.array([2.5]), 0) == 1
    k = PR.known_row(y, 7, 3)
    assert k.rank == 3 and k.row.top_id == [5, 6, 7] and k.logprob == k.row.top_val[2] == 2.0 - k.row.lse
    k = PR.known_row(y, 1, 2)
    assert k.rank == 0 and np.isnan(k.logprob)
    assert np.isnan(PR.known_row(y, 9, 0).logprob)


def test_reference_matches_log_softmax_and_a_sorted_rank():
    g = torch.Generator().manual_seed(9)
    for V in (1, 7, 33, 1000, 4097):
        x = (torch.randn(V, generator=g, dtype=torch.float64) * 3).to(torch.bfloat16).to(torch.float64)      # bf16 values: ties
        want = torch.log_softmax(x, dim=-1)
        desc = torch.sort(x, descending=True).values.numpy()
        for tok in sorted({0, V // 2, V - 1, int(torch.argmax(x)), int(torch.argmin(x))}):
            k = PR.known_row(x.numpy(), tok, min(5, V))
            assert abs(k.logprob - float(want[tok])) < 1e-12
            # in the descending order the token's class ends at position rank: everything before is >=, everything after is smaller
            assert desc[k.rank - 1] == float(x[tok]) and (k.rank == V or desc[k.rank] < float(x[tok]))
            if k.rank <= len(k.row.top_id):
                assert tok in k.row.top_id[:k.rank] and k.row.top_val[k.rank - 1] == k.logprob


def test_the_engine_tests_prompts_need_no_order_excuse_between_the_oracles_own_pipelines():
    """The prompts of tests/test_engine_prompt_logprob_gpu.py: the oracle's token-by-token decode rows against its prefill rows (two
    bf16 pipelines over the same weights) rank the top 5 alike at every prompt position -- well inside that file's cap of 2 %."""
    from oracle.model import Ctx, OracleModel
    from ssd_amd import weights as W
    from tests.test_engine_temperature_gpu import KW, cfgs
    t, _ = cfgs()
    model = OracleModel(t, W.synthetic_state_dict(t, 0, KW["weights_std"]), 16, 16)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)                     # noqa: E731
    bt = i32([list(range(16))])
    total = differs = 0
    with torch.inference_mode():
        for p in PR.ENGINE_PROMPTS + [PR.ENGINE_LONG]:
            T = len(p)
            h = model.forward(torch.tensor(p), torch.arange(T), Ctx("prefill", slot_mapping=torch.arange(T, dtype=torch.int32), cu_q=i32([0, T]), cu_k=i32([0, T])))
            pre = model.compute_logits(h).double()
            for q in range(T - 1):
                ctx = (Ctx("prefill", slot_mapping=i32([0]), cu_q=i32([0, 1]), cu_k=i32([0, 1])) if q == 0 else
                       Ctx("decode", slot_mapping=i32([q]), context_lens=i32([q + 1]), block_tables=bt))
                row = model.compute_logits(model.forward(torch.tensor([p[q]]), torch.tensor([q]), ctx)).double()[0]
                top = lambda r: torch.sort(-r, stable=True).indices[:5].tolist()       # noqa: E731
                differs += top(row) != top(pre[q])
                total += 1
    assert total == sum(len(p) - 1 for p in PR.ENGINE_PROMPTS) + len(PR.ENGINE_LONG) - 1 and differs <= 0.02 * total, (differs, total)


# ---------------------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------------------
def header_symbols():
    return sorted(set(re.findall(r"^int\s+(ssd_\w+)\s*\(", open(HEADER).read(), flags=re.M)))


def test_prompt_logprob_header_symbols_exported_bound_and_documented():
    from ssd_amd.hip.lib import SIGNATURES, ABI_VERSION
    from ssd_amd.hip import logprob_ops, prompt_logprob_ops as P
    _built_lib()
    lib = P.load_prompt_logprob_library()
    syms = header_symbols()
    assert syms == ["ssd_logprob_known_ws_bytes", "ssd_logprob_rows_known"]
    assert sorted(P.PROMPT_LOGPROB_SIGNATURES) == syms
    assert not set(syms) & (set(SIGNATURES) | set(logprob_ops.LOGPROB_SIGNATURES))        # a table of its own
    assert lib.ssd_abi_version() == ABI_VERSION == 3        # additive header: the ABI version does not move
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    head = open(HEADER).read()
    for s in syms:
        assert hasattr(lib, s), f"{s} not exported"
        assert f"`{s}(" in doc, f"{s} has no line in INTEGRATION.md"
        decl = re.search(r"^int\s+" + s + r"\s*\(([^;]*)\);", head, flags=re.M | re.S).group(1)
        assert len(P.PROMPT_LOGPROB_SIGNATURES[s]) == len(decl.split(",")), s
    assert '#include "ssd_hip_logprob.h"' in head and "SSD_LOGPROB_MAX_N" in head and "#define" not in head.split("#define SSD_HIP_PROMPT_LOGPROB_H")[1]
    assert (P.MAX_N, P.MAX_V) == (logprob_ops.MAX_N, logprob_ops.MAX_V)
    assert "rank" in head and "itself included" in head and "NOT read" in head          # the rank's definition, stated where the semantics live
    common = open(os.path.join(ROOT, "ssd_amd", "csrc", "common.h")).read()
    assert '#include "ssd_hip_prompt_logprob.h"' in common
    mk = open(os.path.join(ROOT, "ssd_amd", "csrc", "Makefile")).read()
    assert "../../include/ssd_hip_prompt_logprob.h" in mk and "prompt_logprob.hip" in mk and "logprob.h\n" in mk
    assert P.LAUNCHES == 0                                  # loading and binding launch nothing
    one = P.logprob_known_ws_bytes(1, 4096)
    assert one == logprob_ops.logprob_rows_ws_bytes(1, 4096) and P.logprob_known_ws_bytes(3, 4097) == 6 * one and P.LAUNCHES == 0


def test_c_consumer_walks_every_prompt_logprob_validation_path(tmp_path):
    lib = _built_lib()
    src = os.path.join(ROOT, "tests", "prompt_logprob_abi_consumer.c")
    body = open(src).read()
    for s in header_symbols():
        assert f"{s}(" in body, s
    for what in ("zero T", "negative T", "T above 65535", "zero V", "ld below V", "above SSD_LOGPROB_MAX_V", "null rows", "null n_top",
                 "null tokens", "null lse", "null top_val alone", "null top_id alone", "null out", "null rank", "null ws",
                 "workspace query"):
        assert what in body, what
    exe = str(tmp_path / "prompt_logprob_abi_consumer")
    libdir = os.path.dirname(lib)
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-L", libdir, "-lssdhip",
                    f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "0 failures" in run.stdout


# ---------------------------------------------------------------------------------------------------------------------
# prefix cache: no hit for a sequence whose prompt is still to be scored, but its blocks are there for the next one
# ---------------------------------------------------------------------------------------------------------------------
def test_block_manager_gives_an_asking_sequence_no_hit_but_registers_its_blocks(monkeypatch):
    from ssd_amd.engine.block_manager import BlockManager
    from ssd_amd.engine.sequence import Sequence
    from ssd_amd.sampling_params import SamplingParams
    monkeypatch.setattr(Sequence, "block_size", 4)
    prompt = list(range(1, 11))                             # two full blocks and a partial one
    bm = BlockManager(16, 4)
    first = Sequence(prompt)
    bm.allocate(first)
    assert first.num_cached_tokens == 0 and len(bm.hash_to_block_id) == 2
    asking = Sequence(prompt, SamplingParams(prompt_logprobs=0))
    bm.allocate(asking)
    assert asking.num_cached_tokens == 0                    # the hit is there, and is not taken
    assert not set(asking.block_table) & set(first.block_table) and len(asking.block_table) == 3
    plain = Sequence(prompt)
    bm.allocate(plain)
    assert plain.num_cached_tokens == 8                     # a plain sequence does hit ...
    assert plain.block_table[:2] == asking.block_table[:2]  # ... the blocks the asking one registered last
    # from an empty cache: the asking sequence's own full blocks are hashed and registered
    bm = BlockManager(16, 4)
    asking = Sequence(prompt, SamplingParams(prompt_logprobs=3))
    bm.allocate(asking)
    assert asking.num_cached_tokens == 0 and len(bm.hash_to_block_id) == 2
    plain = Sequence(prompt)
    bm.allocate(plain)
    assert plain.num_cached_tokens == 8 and plain.block_table[:2] == asking.block_table[:2]
    assert [bm.blocks[b].ref_count for b in asking.block_table] == [2, 2, 1]
    # once the records are stored the sequence hits like any other (the re-prefill after a preemption)
    bm.deallocate(asking)
    asking.store_prompt_logprobs([None] + [{"token_id": t} for t in prompt[1:]])
    assert not asking.needs_prompt_logprobs
    bm.allocate(asking)
    assert asking.num_cached_tokens == 8
    # the draft's allocation is untouched: it hits while the records are still missing
    dbm = BlockManager(16, 4, is_draft=True)
    a, b = Sequence(prompt), Sequence(prompt, SamplingParams(prompt_logprobs=0))
    dbm.allocate(a)
    dbm.allocate(b)
    assert b.needs_prompt_logprobs and b.num_draft_cached_tokens == 8 and b.draft_block_table[:2] == a.draft_block_table[:2]


# ---------------------------------------------------------------------------------------------------------------------
# bookkeeping with hand-made records
# ---------------------------------------------------------------------------------------------------------------------
def prec(prompt, N):
    return [None] + [{"token_id": t, "logprob": -t / 100.0, "rank": 1 + t % 3, "top_ids": [t] * min(N, 1), "top_logprobs": [-t / 100.0] * min(N, 1)}
                     for t in prompt[1:]]


class FakeRunner:
    """The runner's side of the contract: run() leaves last_prompt_logprobs for the sequences of a prefill that still need them."""
    def __init__(self):
        self.tok, self.scored, self.last_logprobs = 50, [], None

    def call(self, method, seqs, is_prefill):
        assert method == "run"
        self.last_prompt_logprobs = None
        if is_prefill and any(s.needs_prompt_logprobs for s in seqs):
            self.scored.extend(s.seq_id for s in seqs if s.needs_prompt_logprobs)
            self.last_prompt_logprobs = [prec(s.token_ids, s.prompt_logprobs) if s.needs_prompt_logprobs else None for s in seqs]
        self.tok += len(seqs)
        return list(range(self.tok - len(seqs), self.tok))

    def eagle_acts(self, n):
        raise AssertionError


@pytest.mark.parametrize("speculate", [False, True])
def test_records_are_stored_once_and_survive_a_preemption(speculate):
    from ssd_amd.engine.step import AutoRegressiveStep
    from ssd_amd.engine.verifier import Verifier
    sch = scheduler(speculate)
    asked = new_seq(sch, [1, 2, 3, 4, 5], prompt_logprobs=1, max_new_tokens=8, ignore_eos=True)
    quiet = new_seq(sch, [7, 8, 9], max_new_tokens=8, ignore_eos=True)
    runner = FakeRunner()
    seqs, is_prefill = sch.schedule()
    assert is_prefill and seqs == [asked, quiet]
    if speculate:
        Verifier(3, torch.device("cpu"), runner).prefill(seqs)
    else:
        AutoRegressiveStep(sch, runner).prefill(seqs)
    want = prec([1, 2, 3, 4, 5], 1)
    assert asked.prompt_logprob_records == want and quiet.prompt_logprob_records is None
    assert not asked.needs_prompt_logprobs and runner.scored == [asked.seq_id]
    if speculate:       # (what SpecDecodeStep.prefill and a first round leave behind)
        for s in seqs:
            s.num_cached_tokens = s.num_draft_cached_tokens = s.num_prompt_tokens
            s.append_token(s.recovery_token_id)
    # preempted: the completions become prompt for the scheduler, the records stay those of the request's own prompt
    while sch.running:
        sch.preempt(sch.running.pop())
    assert asked.num_prompt_tokens == 6 and asked.num_request_prompt_tokens == 5
    seqs, is_prefill = sch.schedule()
    assert is_prefill and asked in seqs
    if speculate:
        Verifier(3, torch.device("cpu"), runner).prefill(seqs)
    else:
        AutoRegressiveStep(sch, runner).prefill(seqs)
    assert asked.prompt_logprob_records == want and len(asked.prompt_logprob_records) == asked.num_request_prompt_tokens
    assert runner.scored == [asked.seq_id]                  # the re-prefill did not ask again
    with pytest.raises(AssertionError):
        asked.store_prompt_logprobs(want)                   # never doubled


def test_row_counts_skip_last_rows_and_sequences_that_did_not_ask():
    from ssd_amd.engine.logit_rules import PromptLogprobs
    from ssd_amd.engine.sequence import Sequence
    from ssd_amd.sampling_params import SamplingParams
    a = Sequence([1, 2, 3, 4], SamplingParams(prompt_logprobs=5))
    b = Sequence([1, 2, 3])
    c = Sequence([9], SamplingParams(prompt_logprobs=0))
    d = Sequence([1, 2], SamplingParams(prompt_logprobs=0))
    e = Sequence([1, 2, 3], SamplingParams(prompt_logprobs=2))
    e.store_prompt_logprobs([None, {}, {}])                 # already scored: a re-prefill
    assert PromptLogprobs.row_counts([a, b, c, d, e], [0, 4, 7, 8, 10, 13]) == [5, 5, 5, -1, -1, -1, -1, -1, 0, -1, -1, -1, -1]


def test_generate_returns_the_prompt_records_only_to_those_who_asked(golden, monkeypatch):
    from ssd_amd.engine.step import AutoRegressiveStep
    from ssd_amd.hip import prompt_logprob_ops
    from ssd_amd.sampling_params import SamplingParams
    ar, _ = oracle_engines(golden)
    runner = FakeRunner()
    ar.model_runner.supports_prompt_logprobs = True         # (this test drives the engine with a hand-made runner behind the real step)
    monkeypatch.setattr(ar, "create_inference_step", lambda config: AutoRegressiveStep(ar.scheduler, runner))
    sps = [SamplingParams(temperature=0, max_new_tokens=3, ignore_eos=True, prompt_logprobs=1),
           SamplingParams(temperature=0, max_new_tokens=3, ignore_eos=True),
           SamplingParams(temperature=0, max_new_tokens=3, ignore_eos=True, prompt_logprobs=0)]
    out, _ = ar.generate([[1, 2, 3], [4, 5, 6], [7]], sps, use_tqdm=False)
    asked, quiet, single = out
    assert set(quiet) == {"text", "token_ids", "finish_reason"}              # exactly today's dict
    assert set(asked) == set(quiet) | {"prompt_logprobs"} and asked["prompt_logprobs"] == prec([1, 2, 3], 1)
    assert single["prompt_logprobs"] == [None]
    out2, _ = ar.generate([[1, 2, 3]], sps[1], use_tqdm=False)               # a second generate starts clean
    assert set(out2[0]) == {"text", "token_ids", "finish_reason"}
    assert prompt_logprob_ops.LAUNCHES == 0


def test_runners_without_the_kernel_refuse_prompt_logprobs_by_name(golden):
    from ssd_amd.sampling_params import SamplingParams
    for eng in oracle_engines(golden):
        assert not getattr(eng.model_runner, "supports_prompt_logprobs", False)
        for n in (0, 5):
            with pytest.raises(ValueError, match="prompt_logprobs is not supported"):
                eng.add_request([1, 2, 3], SamplingParams(temperature=0, prompt_logprobs=n))
        assert eng.is_finished()                            # nothing was queued by the refused requests
    ar, _ = oracle_engines(golden)
    ar.model_runner.supports_prompt_logprobs, ar.model_runner.tp_size = True, 2
    with pytest.raises(ValueError, match="prompt_logprobs.*tensor-parallel"):
        ar.add_request([1, 2, 3], SamplingParams(temperature=0, prompt_logprobs=0))
    assert ar.is_finished()


def test_a_default_run_launches_nothing_of_it(golden):
    from ssd_amd.hip import prompt_logprob_ops
    from ssd_amd.sampling_params import SamplingParams
    for eng in oracle_engines(golden):
        out, _ = eng.generate([[1, 2, 3, 4], [5, 6]], SamplingParams(temperature=0, max_new_tokens=4, ignore_eos=True), use_tqdm=False)
        assert all(set(o) == {"text", "token_ids", "finish_reason"} for o in out)
    assert prompt_logprob_ops.LAUNCHES == 0
