"""Characterisation of what the decoder launches: the ordered calls of HipDecoder / HipEagleDraft (ssd_amd/model.py, ssd_amd/eagle.py)
into the op modules, the one-shot collective and torch.distributed, against a recording (tests/golden/decoder_trace.json).

The host side of the decoder decides which kernels a forward launches, with which scalars and over which buffers, for every decoding
mode, quantized target, KV cache format, tensor parallelism and the EAGLE-3 draft; a change there that is meant to leave behaviour
alone must reproduce the recording entry for entry.  No GPU: the decoder is built on torch.device("meta") at the full width of a
preset (three layers), its weights are torch.empty placeholders under the names and shapes of weights.param_shapes (+ "_scale" /
"_zero" / "_bscale" tables), and every launching function of the op modules is replaced by a recorder.  The host-side queries (REAL below) stay
real, so the built library is needed.

An entry is the function and its arguments BOUND TO ITS SIGNATURE, arguments that equal their default left out: passing a default
explicitly or not is no difference.  A tensor argument is described by the buffer it aliases -- the decoder attribute, weight name,
AttnMeta field or scenario input that owns its storage (what _base answers for a plain view, and also for a view through another
dtype, whose _base is an intermediate) -- plus storage offset, dtype and shape: buf_h and buf_res have the same shape and swapping them
fails; kv_cache[li, 0 | 1] and the residual ping-pong show up per layer.

The recording (two files: FIXTURE, and FIXTURE_MORE for the scenarios added since) is written by this file's own record mode,

    python tests/test_decoder_trace_cpu.py --record [--commit HASH]

from the tree whose behaviour is to be pinned (every scenario twice; the two must agree), and is not re-recorded by a change that
claims to leave behaviour alone."""
import contextlib
import dataclasses
import inspect
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "decoder_trace.json")
# scenarios added after the first recording (spec more=True) are kept in a file of their own: a recording is one line of JSON, so
# extending the first file would rewrite all of it, and this way the first recording stays byte for byte what it was
FIXTURE_MORE = os.path.join(ROOT, "tests", "golden", "decoder_trace_more.json")

META = torch.device("meta")
BF16 = torch.bfloat16
OP_MODULES = ("ops", "quant_ops", "fp8b_ops", "w4_ops", "w4zp_ops", "mx4_ops", "kv8_ops", "lora_ops")
# host-side queries: they launch nothing and keep their real implementation (and are not recorded)
REAL = {"frag_numel", "gemm_pf_workspace_bytes", "gemm_argmax_nparts", "chain_segment_ok", "chain_granule_bytes", "tree_segment_ok",
        "tree_segment_workspace_bytes", "fork_topf_workspace_bytes"}
AR_METHODS = ("fits", "fits_rows", "all_reduce", "all_reduce_add_rmsnorm", "all_gather_words")
REQUIRED = {"chain_segment", "tree_segment", "gemm_parts", "rmsnorm_parts", "attn_oproj_parts", "rope_store_kv_parts",
            "gemm_pf", "gemm_fused", "gemm_argmax", "argmax_parts", "argmax_rows", "argmax_rows_val", "argmax_merge", "rmsnorm_pair",
            "gemm_fp8", "gemm_fp8b", "gemm_w4a16", "gemm_w4a16_zp", "gemm_mxfp4",
            "fp8_dequant_frag", "fp8b_dequant_frag", "w4_dequant_frag", "w4zp_dequant_frag", "mx4_dequant_frag",
            "lora_shrink", "lora_expand",
            "rope_store_kv_fp8", "attn_paged_fp8", "all_reduce_add_rmsnorm", "all_gather_words"}
MIN_CALLS = 8

MAX_TOKENS, MAX_MODEL_LEN, BLOCK, KV_BLOCKS, LAYERS = 512, 8192, 16, 64, 3
GRID_PRESETS = ("llama-3.2-1b", "llama-3.2-3b", "llama-3.1-8b", "llama-3.1-70b", "qwen3-0.6b", "qwen3-32b")
GRID_T = (1, 2, 8, 16, 17, 24, 32, 33, 100, 128, 129, 300)


def _scenarios() -> dict:
    """name -> spec.  The part of a name before the first '/' is the group one test case replays."""
    S = {}
    for p in GRID_PRESETS:
        for T in GRID_T:
            for B in (1, 2) if T % 2 == 0 else (1,):
                for ctx in (256, 4096):
                    S[f"grid-{p}/T{T}-B{B}-ctx{ctx}"] = dict(preset=p, T=T, B=B, ctx=ctx)
    for p, T in (("llama-3.2-1b", 24), ("llama-3.1-8b", 100), ("llama-3.1-70b", 100)):
        S[f"modes/varlen-{p}-T{T}"] = dict(preset=p, T=T, B=2, ctx=1024, kind="varlen")
    for p in ("llama-3.2-1b", "qwen3-0.6b", "llama-3.1-8b"):
        S[f"modes/tree-{p}-T24"] = dict(preset=p, T=24, B=2, ctx=1024, kind="tree", out3=p == "llama-3.2-1b")
    quant = {"fp8": dict(quantization="fp8"), "w4a16": dict(quantization="w4a16"), "w4a16zp": dict(quantization="w4a16"),
             "mxfp4": dict(quantization="mxfp4"), "kv8": dict(kv_cache_dtype="fp8"),
             "kv8-w4a16": dict(kv_cache_dtype="fp8", quantization="w4a16")}
    for tag, kw in quant.items():
        for T in (8, 100, 300):
            S[f"quant/{tag}-llama-3.1-8b-T{T}"] = dict(preset="llama-3.1-8b", T=T, B=1, ctx=1024, dec=kw, zero=tag == "w4a16zp")
    for T in (1, 8, 100, 300):
        S[f"quant/kv8-qwen3-0.6b-T{T}"] = dict(preset="qwen3-0.6b", T=T, B=1, ctx=1024, dec=dict(kv_cache_dtype="fp8"))
    for p in ("llama-3.1-8b", "llama-3.2-1b"):
        for T in (1, 8):
            S[f"taps/{p}-T{T}"] = dict(preset=p, T=T, B=1, ctx=1024, dec=dict(taps=[0, 2]))
    for p in ("llama-3.2-3b", "qwen3-0.6b"):
        for sw in ("1", "0"):
            env = dict(SSD_CHAIN_SEG=sw, SSD_TREE_SEG=sw)
            for T in (1, 8, 24):
                S[f"seg/{p}-seg{sw}-T{T}"] = dict(preset=p, T=T, B=1, ctx=1024, env=env)
            S[f"seg/{p}-seg{sw}-tree-T24"] = dict(preset=p, T=24, B=2, ctx=1024, env=env, kind="tree")
    for T in (1, 8, 24):
        S[f"seg/llama-3.2-1b-bias-T{T}"] = dict(preset="llama-3.2-1b", T=T, B=1, ctx=1024, bias=True)
    for T in (1, 8, 100):
        for ar in ("fits", "nofit", None):
            for fused in (True, False):
                S[f"tp/llama-3.1-70b-tp2-ar{ar}-cand{int(fused)}-T{T}"] = dict(
                    preset="llama-3.1-70b", T=T, B=1, ctx=1024, dec=dict(tp_size=2, tp_rank=1), ar=ar, argmax_fused=fused, out2=True)
    for T in (1, 8):
        for ar in ("fits", None):
            S[f"tp/llama-3.1-70b-force-ar{ar}-T{T}"] = dict(preset="llama-3.1-70b", T=T, B=1, ctx=1024, ar=ar, out2=True,
                                                            dec=dict(force_collectives=True, tp_group="group"))
    for p in ("llama-3.2-1b", "llama-3.1-70b"):
        for M in (1, 8):
            S[f"bench/{p}-M{M}"] = dict(preset=p, T=M, kind="bench")
    for T in (1, 8, 40, 300):
        S[f"eagle/eagle3-llama-3.1-8b-T{T}"] = dict(preset="eagle3-llama-3.1-8b", T=T, B=1, ctx=1024, kind="eagle")
    for T in (8, 100, 300):
        S[f"quant/fp8b-llama-3.1-8b-T{T}"] = dict(preset="llama-3.1-8b", T=T, B=1, ctx=1024, dec=dict(quantization="fp8"), bscale=True,
                                                      more=True)
    for tag, kw in (("bf16", {}), ("w4a16", dict(quantization="w4a16"))):
        for T in (8, 100, 300):
            S[f"lora/{tag}-llama-3.1-8b-T{T}"] = dict(preset="llama-3.1-8b", T=T, B=1, ctx=1024, dec=dict(max_loras=2, **kw), lora=True,
                                                            more=True)
    return S


SCENARIOS = _scenarios()
GROUPS = sorted({n.split("/")[0] for n in SCENARIOS})


class _Group:
    """Stand-in for a process group handle (only passed through)."""


def _empty(*shape, dtype=BF16):
    return torch.empty(*shape, dtype=dtype, device=META)


def build_decoder(spec: dict):
    """The decoder of a scenario on the meta device, with placeholder weights and a KV cache."""
    from ssd_amd import quant
    from ssd_amd.eagle import HipEagleDraft
    from ssd_amd.model import HipDecoder
    from ssd_amd.model_config import PRESETS
    from ssd_amd.weights import param_shapes, shard_param
    cfg = PRESETS[spec["preset"]]
    eagle = cfg.family == "eagle3"
    cfg = dataclasses.replace(cfg, num_layers=1 if eagle else LAYERS)
    kw = dict(spec.get("dec", {}))
    if kw.get("tp_group") == "group":
        kw["tp_group"] = _Group()
    dec = (HipEagleDraft if eagle else HipDecoder)(cfg, max_tokens=MAX_TOKENS, max_seqs=2, max_blocks=MAX_MODEL_LEN // BLOCK, block_size=BLOCK,
                                                   max_model_len=MAX_MODEL_LEN, device=META, **kw)
    for name, shape in param_shapes(cfg):
        if name == "d2t":
            dec.target_index = _empty(shape[0], dtype=torch.int64)
            continue
        t = shard_param(cfg, name, _empty(*shape), dec.tp_rank, dec.tp_size)
        if dec.quantized and quant.is_quantized_linear(name):
            N, K = t.shape
            dec.w[name] = _empty(N, K, dtype=torch.uint8)
            if dec.fp8 and spec.get("bscale") and ("qkv_proj" in name or "down_proj" in name):     # block scales on half the linears
                dec.w[name + "_bscale"] = _empty(N // 16, -(-K // quant.FP8_BLOCK), dtype=torch.float32)
            elif dec.fp8:
                dec.w[name + "_scale"] = _empty(N, dtype=torch.float32)
            elif dec.w4:
                dec.w[name + "_scale"] = _empty(N, K // quant.W4_GROUP)
                if spec.get("zero") and ("qkv_proj" in name or "down_proj" in name):       # zero points on half the linears
                    dec.w[name + "_zero"] = _empty(N, K // quant.W4_GROUP, dtype=torch.uint8)
            else:
                dec.w[name + "_scale"] = _empty(N, K // quant.MX4_BLOCK, dtype=torch.uint8)
            continue
        dec.w[name] = t
    if cfg.tie_word_embeddings:
        dec.w["lm_head.weight"] = _empty(dec.V, dec.h)
    if spec.get("bias"):
        for li in range(cfg.num_layers):
            dec.w[f"model.layers.{li}.self_attn.qkv_proj.bias"] = _empty(dec.qkv_n)
    dec.alloc_kv(KV_BLOCKS)
    return dec


class Recorder:
    """Collects entries; names a tensor after the attribute / weight / field / input that owns its storage."""

    def __init__(self):
        self.trace: list[tuple[str, ...]] = []
        self.names: dict[int, str] = {}
        self.keep: list = []

    def name(self, prefix: str, owner) -> None:
        items = owner.items() if isinstance(owner, dict) else vars(owner).items()
        for k, v in sorted(items):
            if isinstance(v, torch.Tensor):
                self.keep.append(v)
                self.names.setdefault(v.untyped_storage()._cdata, prefix.format(k))

    def describe(self, v) -> str:
        if isinstance(v, torch.Tensor):
            who = self.names.get(v.untyped_storage()._cdata)
            assert who is not None, f"a tensor argument aliases no known buffer: {v.dtype} {list(v.shape)}"
            d = f"{who}+{v.storage_offset()}:{str(v.dtype).replace('torch.', '')}{list(v.shape)}"
            return d if v.is_contiguous() else d + f"/{list(v.stride())}"
        if v is None or isinstance(v, (bool, int, float, str)):
            return repr(v)
        if isinstance(v, (list, tuple)):
            return "(" + ",".join(self.describe(x) for x in v) + ")"
        return type(v).__name__

    def wrap(self, tag: str, fn, result=None):
        sig = inspect.signature(fn)

        def recorder(*a, **kw):
            ba = sig.bind(*a, **kw)
            ba.apply_defaults()
            entry = [tag]
            for k, v in ba.arguments.items():
                p = sig.parameters[k]
                if p.default is not inspect.Parameter.empty and (v is p.default or (not isinstance(v, torch.Tensor) and type(v) is type(p.default) and v == p.default)):
                    continue
                entry.append(f"{k}={self.describe(v)}")
            self.trace.append(tuple(entry))
            return result
        return recorder


@contextlib.contextmanager
def recording(rec: Recorder, env: dict):
    """Every launching function of the op modules and ssd_amd.model's torch.distributed replaced by recorders; SSD_CHAIN_SEG /
    SSD_TREE_SEG as the scenario sets them (unset otherwise)."""
    import importlib
    import types
    import ssd_amd.model as model
    saved, saved_env = [], {k: os.environ.pop(k, None) for k in ("SSD_CHAIN_SEG", "SSD_TREE_SEG")}
    os.environ.update(env)
    try:
        for short in OP_MODULES:
            mod = importlib.import_module("ssd_amd.hip." + short)
            for name, fn in list(vars(mod).items()):
                if (name.startswith("_") or name.startswith("load_") or name in REAL or not inspect.isfunction(fn)
                        or fn.__module__ != mod.__name__):
                    continue
                saved.append((mod, name, fn))
                setattr(mod, name, rec.wrap(f"{short}.{name}", fn))
        dist = model.dist
        saved.append((model, "dist", dist))
        model.dist = types.SimpleNamespace(all_reduce=rec.wrap("dist.all_reduce", dist.all_reduce),
                                           all_gather_into_tensor=rec.wrap("dist.all_gather_into_tensor", dist.all_gather_into_tensor))
        yield
    finally:
        for owner, name, fn in saved:
            setattr(owner, name, fn)
        for k, v in saved_env.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def stand_in_ar(rec: Recorder, fits: bool):
    """An object with the recorded methods of utils/custom_ar.py OneShotAllReduce (signatures taken from the class)."""
    import types
    from ssd_amd.utils.custom_ar import OneShotAllReduce
    ar = types.SimpleNamespace()
    for m in AR_METHODS:
        fn = getattr(OneShotAllReduce, m)
        sig = inspect.signature(fn)

        def bare(*a, **kw):
            raise AssertionError("never called")
        bare.__signature__ = sig.replace(parameters=list(sig.parameters.values())[1:])        # without self
        setattr(ar, m, rec.wrap(f"ar.{m}", bare, result=fits if m.startswith("fits") else None))
    return ar


def run_scenario(name: str) -> list[tuple[str, ...]]:
    """One decoder, one forward + compute_logits + argmax (or bench.py's four calls / the draft's project + forward + head)."""
    from ssd_amd.hip import ops as H
    from ssd_amd.model import AttnMeta
    spec = SCENARIOS[name]
    rec = Recorder()
    kind, T = spec.get("kind", "step"), spec["T"]
    with recording(rec, spec.get("env", {})):
        dec = build_decoder(spec)
        if spec.get("ar"):
            dec.custom_ar = stand_in_ar(rec, spec["ar"] == "fits")
        if "argmax_fused" in spec:
            dec.argmax_fused = spec["argmax_fused"]
        i32 = lambda *s: _empty(*s, dtype=torch.int32)      # noqa: E731
        inp = dict(input_ids=_empty(T, dtype=torch.int64), positions=_empty(T, dtype=torch.int64))
        if kind == "bench":
            inp["slots"] = i32(T)
            rec.name("{}", inp), rec.name("w[{}]", dec.w), rec.name("{}", dec)
            for li in (0, 1):
                dec.launch_qkv(li, T, inp["positions"], inp["slots"], gemm_only=True)
                dec.launch_o(li, T)
                dec.launch_gate_up(li, T, gemm_only=True)
                dec.launch_down(li, T)
            return rec.trace
        B = spec["B"]
        bt = i32(B, dec.max_blocks)
        if kind == "varlen":
            meta = AttnMeta(H.MODE_CAUSAL, B, T - T // 3, i32(T), i32(B), bt, cu_q=i32(B + 1), ctx_hint=spec["ctx"])
        elif kind == "tree":
            meta = AttnMeta(H.MODE_TREE, B, T // B, i32(T), i32(B), bt, q_per_seq=T // B, tree_K=3, tree_mq=T // B, tree_step=1, tree_F=1,
                            tree_jidx=i32(B, 4), ctx_hint=spec["ctx"])
        else:
            meta = AttnMeta(H.MODE_CAUSAL, B, T // B, i32(T), i32(B), bt, q_per_seq=T // B, ctx_hint=spec["ctx"])
        gather = T > 32 or kind == "varlen"
        n = B if gather else T
        inp.update(out=_empty(n, dtype=torch.int64), out2=_empty(n, dtype=torch.int64), out3=_empty(n, 3, dtype=torch.int64),
                   gather=i32(B), acts_rows=_empty(T, getattr(dec, "A", 1)))
        rec.name("{}", inp), rec.name("meta.{}", meta), rec.name("w[{}]", dec.w), rec.name("{}", dec)
        if spec.get("lora"):        # an adapted row in the batch: every linear takes the ROWS route and adds its delta
            dec.lora_active = True
            rec.name("lora_a[{}]", dec.lora_a), rec.name("lora_b[{}]", dec.lora_b)
        if kind == "eagle":
            dec.project(inp["acts_rows"], T, dec.buf_cond)
        dec.forward(inp["input_ids"], inp["positions"], T, meta)
        if gather:
            dec.compute_logits(T, gather=inp["gather"], rows=B)
        else:
            dec.compute_logits(T)
        if spec.get("out3"):
            dec.argmax(n, inp["out"], inp["out2"], inp["out3"], 3)
        elif spec.get("out2"):
            dec.argmax(n, inp["out"], inp["out2"])
        else:
            dec.argmax(n, inp["out"])
    return rec.trace


def _show(entry) -> str:
    return f"{entry[0]}({', '.join(entry[1:])})"


@pytest.fixture(scope="module")
def recorded():
    """name -> the recorded entries of every scenario, from both files."""
    out = {}
    for path, more in ((FIXTURE, False), (FIXTURE_MORE, True)):
        with open(path) as f:
            fx = json.load(f)
        decoded = [tuple(fx["atoms"][i] for i in e) for e in fx["entries"]]
        assert set(fx["scenarios"]) == {n for n, spec in SCENARIOS.items() if bool(spec.get("more")) == more}, path
        out.update({name: [decoded[i] for i in idx] for name, idx in fx["scenarios"].items()})
    return out


def test_recording_is_not_hollow(recorded):
    assert os.path.getsize(FIXTURE) < 1 << 20 and os.path.getsize(FIXTURE_MORE) < 1 << 20
    assert set(recorded) == set(SCENARIOS)
    seen = set()
    for name, entries in recorded.items():
        assert len(entries) >= MIN_CALLS, f"{name}: only {len(entries)} calls recorded"
        seen.update(e[0].split(".", 1)[1] for e in entries)
    assert not REQUIRED - seen, f"never recorded: {sorted(REQUIRED - seen)}"


@pytest.mark.parametrize("group", GROUPS)
def test_decoder_launches_are_the_recorded_ones(recorded, group):
    for name in (n for n in SCENARIOS if n.split("/")[0] == group):
        want = recorded[name]
        got = run_scenario(name)
        for i, (a, b) in enumerate(zip(got, want)):
            assert a == b, (f"{name}: call {i} differs from the recording\n  got      {_show(a)}\n  recorded {_show(b)}\n"
                            f"  after    {[_show(e) for e in got[max(0, i - 3):i]]}")
        assert len(got) == len(want), f"{name}: {len(got)} calls, {len(want)} recorded"


def record(commit: str) -> None:
    """Run every scenario twice (the two recordings must agree) and write the two fixtures, each a table of distinct strings, a
    table of distinct entries as indices into it, and one index list per scenario of its own."""
    seen = set()
    first = os.environ.get("DECODER_TRACE_OUT", FIXTURE)
    for out, more in ((first, False), (first[:-len(".json")] + "_more.json", True)):
        atoms, atom_ix, entries, entry_ix, scenarios = [], {}, [], {}, {}
        for name in (n for n, spec in SCENARIOS.items() if bool(spec.get("more")) == more):
            a, b = run_scenario(name), run_scenario(name)
            assert a == b, f"{name}: the two recordings differ"
            assert len(a) >= MIN_CALLS, f"{name}: only {len(a)} calls"
            idx = []
            for e in a:
                if e not in entry_ix:
                    for s in e:
                        if s not in atom_ix:
                            atom_ix[s] = len(atoms)
                            atoms.append(s)
                    entry_ix[e] = len(entries)
                    entries.append([atom_ix[s] for s in e])
                idx.append(entry_ix[e])
            scenarios[name] = idx
        seen |= {e[0].split(".", 1)[1] for e in entry_ix}
        with open(out, "w") as f:
            json.dump({"recorded_at": commit, "atoms": atoms, "entries": entries, "scenarios": scenarios}, f, separators=(",", ":"))
            f.write("\n")
        print(f"wrote {out}: {len(scenarios)} scenarios, {sum(map(len, scenarios.values()))} calls, {len(entries)} distinct entries, "
              f"{len(atoms)} distinct strings, {os.path.getsize(out)} bytes")
    assert not REQUIRED - seen, f"never reached: {sorted(REQUIRED - seen)}"


if __name__ == "__main__":
    assert "--record" in sys.argv, "usage: python tests/test_decoder_trace_cpu.py --record [--commit HASH]"
    record(sys.argv[sys.argv.index("--commit") + 1] if "--commit" in sys.argv else "unknown")
