"""top_k / top_p / min_p, the parts that need no GPU: SamplingParams and Sequence, the async wire block, the refusal by runners that
cannot truncate, the float64 restatement's own hand-checked rows, and the C ABI of include/ssd_hip_filter.h (export, ctypes table,
INTEGRATION.md, a plain-C consumer walking the argument validation)."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests import filter_ref as R

HEADER = os.path.join(ROOT, "include", "ssd_hip_filter.h")


# ---------------------------------------------------------------------------------------------------------------------
# public interface
# ---------------------------------------------------------------------------------------------------------------------
def test_sampling_params_defaults_are_off_and_values_are_validated():
    from ssd_amd.sampling_params import SamplingParams
    from ssd_amd.engine.sequence import Sequence
    sp = SamplingParams()
    assert (sp.top_k, sp.top_p, sp.min_p) == (0, 1.0, 0.0) and sp.active_filters == []
    assert (sp.temperature, sp.draft_temperature, sp.max_new_tokens, sp.ignore_eos) == (1.0, None, 256, False)
    s = Sequence([1, 2, 3], sp)
    assert (s.top_k, s.top_p, s.min_p) == (0, 1.0, 0.0) and not s.has_filter
    assert not Sequence([1]).has_filter
    sp = SamplingParams(temperature=0.7, top_k=50, top_p=0.9, min_p=0.05)
    assert sp.active_filters == ["top_k", "top_p", "min_p"]
    s = Sequence([1, 2, 3], sp)
    assert (s.top_k, s.top_p, s.min_p) == (50, 0.9, 0.05) and s.has_filter
    assert SamplingParams(top_p=1.0, min_p=1.0, top_k=1).active_filters == ["top_k", "min_p"]
    assert SamplingParams(top_p=1e-6).active_filters == ["top_p"]
    for bad in (dict(top_k=-1), dict(top_k=1.5), dict(top_k=True), dict(top_p=0.0), dict(top_p=-0.1), dict(top_p=1.01),
                dict(top_p=float("nan")), dict(min_p=-0.01), dict(min_p=1.5), dict(min_p=float("nan"))):
        name = next(iter(bad))
        with pytest.raises(ValueError, match=name):
            SamplingParams(**bad)


def test_wire_round_trip_with_and_without_the_filter_block():
    from ssd_amd.engine import async_proto as P
    assert P.FLAG_FILTER == 4 and not P.FLAG_FILTER & (P.FLAG_WANT_LOGITS | P.FLAG_EAGLE)
    keys = [(7, -2, 11), (8, 2, 5)]
    nts, tables, temps, mb = [9, 14], [[3, 4], [5]], [0.7, 0.0], 3
    # today's payload, field by field: nothing of the feature without the keyword (or with filters=None)
    today = [7, -2, 11, 8, 2, 5, 9, 14, 3, 4, -1, 5, -1, -1, P.temp_bits(0.7), P.temp_bits(0.0)]
    assert P.pack_speculate(keys, nts, tables, temps, mb) == today
    assert P.pack_speculate(keys, nts, tables, temps, mb, filters=None) == today
    assert P.unpack_speculate(today, 2, mb) == (keys, nts, [[3, 4, -1], [5, -1, -1]], [P.bits_temp(P.temp_bits(0.7)), 0.0])
    filters = ([50, 0], [0.9, 1.0], [0.0, 0.05])
    pl = P.pack_speculate(keys, nts, tables, temps, mb, filters=filters)
    assert pl[:len(today)] == today and len(pl) == len(today) + 3 * 2
    assert pl[len(today):len(today) + 2] == [50, 0]
    *head, got = P.unpack_speculate(pl, 2, mb, filters=True)
    assert tuple(head) == P.unpack_speculate(today, 2, mb)
    f32 = lambda v: float(np.float32(v))
    assert got == ([50, 0], [f32(0.9), 1.0], [0.0, f32(0.05)])
    # with the EAGLE extend block the filter block still comes last
    ext = P.pack_speculate(keys, nts, tables, temps, mb, [1, 0], [[4, 0], [0, 0]], filters=filters)
    plain = P.pack_speculate(keys, nts, tables, temps, mb, [1, 0], [[4, 0], [0, 0]])
    assert ext[:len(plain)] == plain
    *head, got2 = P.unpack_speculate(ext, 2, mb, 2, filters=True)
    assert tuple(head) == P.unpack_speculate(plain, 2, mb, 2) and got2 == got


class _Link:
    """Records what SpeculatorAsync hands to AsyncLink.speculate."""
    def __init__(self, K):
        self.K, self.calls = K, []

    def speculate(self, keys, nts, tables, temps, **kw):
        self.calls.append(kw)
        return [0] * len(keys), [[1] * self.K for _ in keys], None


def test_speculator_async_sends_the_block_only_when_some_sequence_has_a_filter():
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
    assert "filters" not in link.calls[-1]
    spec.speculate(seqs([SamplingParams(temperature=0.7), SamplingParams(temperature=0.7, top_p=0.9)]), VerifyResult([], [], None))
    assert link.calls[-1]["filters"] == ([0, 0], [1.0, 0.9], [0.0, 0.0])


def test_runners_without_the_filter_refuse_a_filtered_request_by_name(golden):
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
        assert not getattr(eng.model_runner, "supports_logit_filters", False)
        for kw, name in ((dict(top_k=5), "top_k"), (dict(top_p=0.9), "top_p"), (dict(min_p=0.1), "min_p"), (dict(top_p=0.9, min_p=0.1), "top_p")):
            with pytest.raises(ValueError, match=name):
                eng.add_request([1, 2, 3], SamplingParams(temperature=0.8, **kw))
        assert eng.is_finished()                       # nothing was queued by the refused requests
    # the defaults are not a filter: the request is taken
    ar.add_request([1, 2, 3], SamplingParams(temperature=0, max_new_tokens=2, ignore_eos=True))
    assert not ar.is_finished()
    from ssd_amd.engine.model_runner import ModelRunner
    from ssd_amd.engine.eagle_runner import EagleDraftRunner
    assert ModelRunner.supports_logit_filters and EagleDraftRunner.supports_logit_filters


# ---------------------------------------------------------------------------------------------------------------------
# the reference itself, on rows small enough to check by hand
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_on_hand_made_rows():
    T = 1.0 / np.log(2.0)
    x = np.array([0.0, -1, -2, -3, -4, -5, -6, -6])          # probabilities 1/2, 1/4, ... 1/128, 1/128
    assert R.filter_row(x, T, top_p=0.7).keep.tolist() == [True, True] + [False] * 6
    assert R.filter_row(x, T, top_k=3).keep.sum() == 3
    assert R.filter_row(x, T, top_k=7).keep.sum() == 8          # the tie at the 7th / 8th place is kept whole
    assert R.filter_row(x, T, min_p=0.1).keep.sum() == 4          # 1/16 of the largest is below 0.1
    assert R.filter_row(x, T, top_k=2, top_p=0.7).keep.sum() == 2          # 0.7 of the mass of K = {1/2, 1/4} needs both
    assert R.filter_row(x, T, top_k=2, top_p=0.6).keep.sum() == 1
    for kw in (dict(), dict(top_k=8), dict(top_k=100)):
        r = R.filter_row(x, T, **kw)
        assert not r.touched and r.keep.all()
    assert not R.filter_row(x, 0.0, top_k=2, top_p=0.5, min_p=0.5).touched
    y = np.array([1.0, np.nan, 0.0, -0.0, -np.inf, 3.0, 3.0, 2.0])
    assert R.filter_row(y, 1.0, top_k=1).keep.tolist() == [False] * 5 + [True, True, False]
    assert R.filter_row(y, 1.0, top_k=5).keep.tolist() == [True, False, True, True, False, True, True, True]          # -0.0 ties +0.0
    assert R.filter_row(y, 1.0, top_p=1e-6).keep.sum() == 2 and R.filter_row(y, 1.0, min_p=1.0).keep.sum() == 2
    assert not R.filter_row(np.full(4, np.nan), 1.0, top_k=1).touched
    p = R.renormalised(R.filter_row(x, T, top_k=2))
    assert np.allclose(p[:2], [2 / 3, 1 / 3]) and p[2:].sum() == 0


# ---------------------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------------------
def _built_lib():
    from ssd_amd.hip.lib import build_library, lib_path
    if not os.path.exists(lib_path()):
        build_library()
    return lib_path()


def filter_header_symbols():
    return sorted(set(re.findall(r"^int\s+(ssd_\w+)\s*\(", open(HEADER).read(), flags=re.M)))


def test_filter_header_symbols_exported_bound_and_documented():
    from ssd_amd.hip.lib import SIGNATURES, ABI_VERSION
    from ssd_amd.hip import filter_ops
    _built_lib()
    lib = filter_ops.load_filter_library()
    syms = filter_header_symbols()
    assert syms == ["ssd_filter_rows"] and sorted(filter_ops.FILTER_SIGNATURES) == syms
    assert not set(syms) & set(SIGNATURES)             # lib.SIGNATURES stays exactly ssd_hip.h + ssd_hip_tune.h
    assert lib.ssd_abi_version() == ABI_VERSION == 3   # additive header: the ABI version does not move
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    head = open(HEADER).read()
    for s in syms:
        assert hasattr(lib, s), f"{s} not exported"
        assert f"`{s}(" in doc, f"{s} has no line in INTEGRATION.md"
        decl = re.search(r"^int\s+" + s + r"\s*\(([^;]*)\);", head, flags=re.M | re.S).group(1)
        assert len(filter_ops.FILTER_SIGNATURES[s]) == len(decl.split(",")), s
    assert int(re.search(r"#define SSD_FILTER_MAX_V (\d+)", head).group(1)) == filter_ops.MAX_V >= 196608
    common = open(os.path.join(ROOT, "ssd_amd", "csrc", "common.h")).read()
    assert '#include "ssd_hip_filter.h"' in common
    mk = open(os.path.join(ROOT, "ssd_amd", "csrc", "Makefile")).read()
    assert mk.count("../../include/ssd_hip_filter.h") == 2 and " filter.hip" in mk
    assert filter_ops.LAUNCHES == 0                    # loading and binding launch nothing


def test_c_consumer_walks_the_filter_validation_paths(tmp_path):
    lib = _built_lib()
    src = os.path.join(ROOT, "tests", "filter_abi_consumer.c")
    body = open(src).read()
    for s in filter_header_symbols():
        assert f"{s}(" in body, s
    for what in ("zero T", "zero V", "zero rows_per_param", "ld below V", "above SSD_FILTER_MAX_V", "null rows", "null temps",
                 "null top_k", "null top_p", "null min_p"):
        assert what in body
    exe = str(tmp_path / "filter_abi_consumer")
    libdir = os.path.dirname(lib)
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-L", libdir, "-lssdhip",
                    f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "0 failures" in run.stdout
