"""Per-request seeds, the parts that need no GPU: the stream's known answers in the numpy restatement, SamplingParams and Sequence,
the Sampling value and its graph names, the async wire block, the refusal by runners without the stream, and the C ABI of
include/ssd_hip_seed.h (export, ctypes table, INTEGRATION.md, a plain-C consumer walking the argument validation)."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests import seed_ref as R

HEADER = os.path.join(ROOT, "include", "ssd_hip_seed.h")


# ---------------------------------------------------------------------------------------------------------------------
# the stream
# ---------------------------------------------------------------------------------------------------------------------
def test_known_answers_of_the_stream():
    assert int(R.key(0, 1, 0)) == 0x9c8c1ca9370e13af and int(R.key(0, 2, 0)) == 0xc83312cb7bd81b65
    for (seed, purpose, pos, idx), want in (((0, 1, 0, 0), 2331386), ((0, 2, 0, 0), 10258722), ((42, 2, 9, 5), 9468248),
                                            ((2 ** 63 - 1, 3, 8191, 0), 11556502), ((1234567890123, 1, 300, 128255), 9889909)):
        assert int(R.bits24(seed, purpose, pos, idx)) == want, (seed, purpose, pos, idx)
    u = R.uniform(0, 1, 0, 0)
    assert u.dtype == np.float32 and float(u).hex() == "0x1.1c97d40000000p-3"
    # the header states the same definition and the same answers
    head = open(HEADER).read()
    for word in ("0x9c8c1ca9370e13af", "0xc83312cb7bd81b65", "2331386", "10258722", "9468248", "11556502", "9889909", "0x1.1c97d4p-3",
                 "0x9e3779b97f4a7c15", "0xbf58476d1ce4e5b9", "0x94d049bb133111eb"):
        assert word in head, word
    assert (R.DRAFT, R.TARGET, R.ACCEPT) == tuple(int(re.search(rf"#define SSD_SEED_{n} (\d+)", head).group(1))
                                                  for n in ("DRAFT", "TARGET", "ACCEPT"))
    # broadcasting, and (0, 1): 24 bits
    grid = R.uniform(np.arange(4, dtype=np.uint64)[:, None], R.TARGET, 7, np.arange(1000, dtype=np.uint64)[None, :])
    assert grid.shape == (4, 1000) and (grid > 0).all() and (grid <= 1).all() and len(np.unique(grid)) > 3900


# ---------------------------------------------------------------------------------------------------------------------
# public interface
# ---------------------------------------------------------------------------------------------------------------------
def test_sampling_params_seed_is_off_by_default_and_validated():
    from ssd_amd.sampling_params import SamplingParams
    from ssd_amd.engine.sequence import Sequence
    assert SamplingParams().seed is None and Sequence([1, 2]).seed is None
    for ok in (0, 1, 7, 2 ** 63 - 1):
        assert Sequence([1, 2, 3], SamplingParams(seed=ok)).seed == ok
    for bad in (True, False, -1, 2 ** 63, 1.0, 1.5, "7", float("nan")):
        with pytest.raises(ValueError, match="seed"):
            SamplingParams(seed=bad)


def test_sampling_value_names_only_seeded_graphs_differently():
    from ssd_amd.engine.model_runner import Sampling, GREEDY
    assert GREEDY.seed is False and GREEDY.suffix == ""
    assert Sampling(True).suffix == "_s" and Sampling(True, True, True, True).suffix == "_sf_p_l"       # what the launch trace pins
    assert Sampling(True, seed=True).suffix == "_s_d" and Sampling(True, True, True, True, True).suffix == "_sf_p_l_d"
    assert Sampling.explicit([0.7, 0.0], None) == Sampling(True)
    assert Sampling.explicit([0.7, 0.0], None, [-1, -1]) == Sampling(True)
    assert Sampling.explicit([0.7, 0.0], None, [-1, 5]) == Sampling(True, seed=True)
    assert Sampling.explicit([0.0, 0.0], None, [3, 5]) == GREEDY                 # no effect at temperature 0
    assert Sampling.explicit(None, None, [3]) == GREEDY


def test_wire_round_trip_with_and_without_the_seed_block():
    from ssd_amd.engine import async_proto as P
    assert P.FLAG_SEED == 8 and not P.FLAG_SEED & (P.FLAG_WANT_LOGITS | P.FLAG_EAGLE | P.FLAG_FILTER)
    keys = [(7, -2, 11), (8, 2, 5)]
    nts, tables, temps, mb = [9, 14], [[3, 4], [5]], [0.7, 0.0], 3
    today = [7, -2, 11, 8, 2, 5, 9, 14, 3, 4, -1, 5, -1, -1, P.temp_bits(0.7), P.temp_bits(0.0)]
    assert P.pack_speculate(keys, nts, tables, temps, mb) == today
    assert P.pack_speculate(keys, nts, tables, temps, mb, seeds=None) == today
    seeds = [2 ** 63 - 1, -1]
    pl = P.pack_speculate(keys, nts, tables, temps, mb, seeds=seeds)
    assert pl == today + seeds
    assert np.array(pl, dtype=np.int64).tolist() == pl                  # every word fits the int64 message
    *head, got = P.unpack_speculate(pl, 2, mb, seeds=True)
    assert tuple(head) == P.unpack_speculate(today, 2, mb) and got == seeds
    # behind the filter block, which stays where it was; and behind the EAGLE extend block
    filters = ([50, 0], [0.9, 1.0], [0.0, 0.05])
    with_f = P.pack_speculate(keys, nts, tables, temps, mb, filters=filters)
    both = P.pack_speculate(keys, nts, tables, temps, mb, filters=filters, seeds=[0, 12345678901234567])
    assert both == with_f + [0, 12345678901234567]
    *head, f, s = P.unpack_speculate(both, 2, mb, filters=True, seeds=True)
    assert tuple(head) + (f,) == P.unpack_speculate(with_f, 2, mb, filters=True) and s == [0, 12345678901234567]
    plain = P.pack_speculate(keys, nts, tables, temps, mb, [1, 0], [[4, 0], [0, 0]])
    ext = P.pack_speculate(keys, nts, tables, temps, mb, [1, 0], [[4, 0], [0, 0]], seeds=seeds)
    assert ext == plain + seeds
    *head, s = P.unpack_speculate(ext, 2, mb, 2, seeds=True)
    assert tuple(head) == P.unpack_speculate(plain, 2, mb, 2) and s == seeds


class _Link:
    """Records what SpeculatorAsync hands to AsyncLink.speculate."""
    def __init__(self, K):
        self.K, self.calls = K, []

    def speculate(self, keys, nts, tables, temps, **kw):
        self.calls.append(kw)
        return [0] * len(keys), [[1] * self.K for _ in keys], None


def test_speculator_async_sends_the_block_only_when_some_sequence_has_a_seed():
    import torch
    from ssd_amd.engine.sequence import Sequence
    from ssd_amd.engine.speculate_types import VerifyResult
    from ssd_amd.engine.speculator_async import SpeculatorAsync
    from ssd_amd.sampling_params import SamplingParams

    def seqs(sps):
        out = []
        for sp in sps:
            s = Sequence([1, 2, 3], sp)
            s.recovery_token_id = 4
            out.append(s)
        return out
    link = _Link(2)
    spec = SpeculatorAsync(2, torch.device("cpu"), link, None)
    spec.speculate(seqs([SamplingParams(temperature=0.7), SamplingParams(temperature=0)]), VerifyResult([], [], None))
    assert "seeds" not in link.calls[-1] and "filters" not in link.calls[-1]
    spec.speculate(seqs([SamplingParams(temperature=0.7), SamplingParams(temperature=0.7, seed=9)]), VerifyResult([], [], None))
    assert link.calls[-1]["seeds"] == [-1, 9] and "filters" not in link.calls[-1]
    spec.speculate(seqs([SamplingParams(temperature=0.7, top_k=4, seed=0)]), VerifyResult([], [], None))
    assert link.calls[-1]["seeds"] == [0] and link.calls[-1]["filters"] == ([4], [1.0], [0.0])


def test_runners_without_the_stream_refuse_a_seeded_request_by_name(golden):
    from oracle.runner import oracle_runner_factory
    from ssd_amd.engine.llm_engine import LLMEngine
    from ssd_amd.sampling_params import SamplingParams
    from tests.test_engine_cpu import mcfg, weights, COMMON
    g = golden("engine_golden")
    wt, wd = weights(g, "t."), weights(g, "d.")
    ar = LLMEngine("tiny", hf_config=mcfg(g, "t_"), runner_factory=oracle_runner_factory(wt), **COMMON)
    sd = LLMEngine("tiny", hf_config=mcfg(g, "t_"), draft="tiny-draft", draft_hf_config=mcfg(g, "d_"), speculate=True, speculate_k=3,
                   runner_factory=oracle_runner_factory(wt, wd), **COMMON)
    for eng in (ar, sd):
        assert not getattr(eng.model_runner, "supports_seed", False)
        for kw in (dict(temperature=0.8, seed=1), dict(temperature=0, seed=1)):
            with pytest.raises(ValueError, match="seed"):
                eng.add_request([1, 2, 3], SamplingParams(**kw))
        assert eng.is_finished()                       # nothing was queued by the refused requests
    ar.add_request([1, 2, 3], SamplingParams(temperature=0, max_new_tokens=2, ignore_eos=True))     # no seed: taken as ever
    assert not ar.is_finished()
    from ssd_amd.engine.model_runner import ModelRunner
    from ssd_amd.engine.eagle_runner import EagleDraftRunner
    assert ModelRunner.supports_seed and EagleDraftRunner.supports_seed


# ---------------------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------------------
def _built_lib():
    from ssd_amd.hip.lib import build_library, lib_path
    if not os.path.exists(lib_path()):
        build_library()
    return lib_path()


def seed_header_symbols():
    return sorted(set(re.findall(r"^(?:int|long)\s+(ssd_\w+)\s*\(", open(HEADER).read(), flags=re.M)))


def test_seed_header_symbols_exported_bound_and_documented():
    from ssd_amd.hip.lib import SIGNATURES, ABI_VERSION
    from ssd_amd.hip import seed_ops
    _built_lib()
    lib = seed_ops.load_seed_library()
    syms = seed_header_symbols()
    assert syms == ["ssd_sample_rows_seeded", "ssd_sample_seeded_ws_bytes", "ssd_seeded_uniforms", "ssd_verify_ratio_seeded"]
    assert sorted(seed_ops.SEED_SIGNATURES) == syms
    assert not set(syms) & set(SIGNATURES)             # lib.SIGNATURES stays exactly ssd_hip.h + ssd_hip_tune.h
    assert lib.ssd_abi_version() == ABI_VERSION == 3   # additive header: the ABI version does not move
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    head = open(HEADER).read()
    main = open(os.path.join(ROOT, "include", "ssd_hip.h")).read()
    for s in syms:
        assert hasattr(lib, s), f"{s} not exported"
        assert f"`{s}(" in doc, f"{s} has no line in INTEGRATION.md"
        decl = re.search(r"^(?:int|long)\s+" + s + r"\s*\(([^;]*)\);", head, flags=re.M | re.S).group(1)
        assert len(seed_ops.SEED_SIGNATURES[s]) == len(decl.split(",")), s
    # "takes the arguments of" the unseeded entry points: the leading arguments are theirs, in their order
    for new, old in (("ssd_sample_rows_seeded", "ssd_sample_rows"), ("ssd_verify_ratio_seeded", "ssd_verify_ratio")):
        was = len(re.search(r"^int\s+" + old + r"\s*\(([^;]*)\);", main, flags=re.M | re.S).group(1).split(","))
        assert seed_ops.SEED_SIGNATURES[new][:was] == SIGNATURES[old], new
    assert (seed_ops.DRAFT, seed_ops.TARGET, seed_ops.ACCEPT) == (R.DRAFT, R.TARGET, R.ACCEPT)
    assert int(re.search(r"#define SSD_SEED_SLICE (\d+)", head).group(1)) == seed_ops.SLICE == 4096
    common = open(os.path.join(ROOT, "ssd_amd", "csrc", "common.h")).read()
    assert '#include "ssd_hip_seed.h"' in common
    mk = open(os.path.join(ROOT, "ssd_amd", "csrc", "Makefile")).read()
    assert "../../include/ssd_hip_seed.h" in mk and "seeded.hip" in mk
    assert seed_ops.LAUNCHES == 0                      # loading and binding launch nothing
    # the workspace query answers on the host, for every shape the unseeded sampler takes
    one = seed_ops.sample_seeded_ws_bytes(1, 4096)
    assert one == 8 and seed_ops.sample_seeded_ws_bytes(3, 4097) == 6 * one and seed_ops.sample_seeded_ws_bytes(1, 1) == one
    assert seed_ops.sample_seeded_ws_bytes(2 ** 31 - 1, 2 ** 31 - 1) == (2 ** 31 - 1) * 2 ** 19 * 8 and seed_ops.LAUNCHES == 0


def test_one_definition_of_the_hash_and_of_the_ratio_verification():
    """csrc/stochastic.h holds mix64, both streams and the verify kernel; neither .hip file restates them."""
    src = {n: open(os.path.join(ROOT, "ssd_amd", "csrc", n)).read() for n in ("stochastic.h", "stochastic.hip", "seeded.hip")}
    assert src["stochastic.h"].count("uint64_t mix64(") == 1 and src["stochastic.h"].count("verify_ratio_kernel(") == 1
    for n in ("stochastic.hip", "seeded.hip"):
        assert '#include "stochastic.h"' in src[n] and "0x9e3779b97f4a7c15" not in src[n] and "mix64(uint64_t" not in src[n]
    assert "verify_ratio_kernel<false>" in src["stochastic.hip"] and "verify_ratio_kernel<true>" in src["seeded.hip"]


def test_c_consumer_walks_every_seed_validation_path(tmp_path):
    lib = _built_lib()
    src = os.path.join(ROOT, "tests", "seed_abi_consumer.c")
    body = open(src).read()
    for s in seed_header_symbols():
        assert f"{s}(" in body, s
    for what in ("zero T", "zero V", "zero rows_per_temp", "zero rows_per_seed", "null rows", "null temps", "null rng", "null out",
                 "null row_seed", "null positions", "null workspace", "purpose 0", "purpose 4", "boost_k 9", "zero B", "zero K", "K 63",
                 "zero rows", "zero n", "index past 2^32", "workspace query"):
        assert what in body, what
    exe = str(tmp_path / "seed_abi_consumer")
    libdir = os.path.dirname(lib)
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-L", libdir, "-lssdhip",
                    f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "0 failures" in run.stdout
