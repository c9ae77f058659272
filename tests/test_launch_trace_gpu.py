"""Characterisation of what the runners launch: the ordered calls into ssd_amd.hip.ops / filter_ops / penalty_ops of short engine
runs, and the hipGraphs those runs create, against a recording (tests/golden/launch_trace.json).

The host side of engine/model_runner.py and engine/eagle_runner.py decides which kernels run, in which order and with which scalar
arguments; a change there that is meant to leave behaviour alone must reproduce the recording entry for entry.  Sixteen runs: the
tiny Llama of tests/golden/tiny_llama.npz as target and as its own draft, two sequences, speculate_k = 3, 6 new tokens, in three
modes (autoregressive, synchronous speculation, asynchronous speculation over the in-process loopback) times five sampling settings,
one asynchronous run under sampler_x (the boosted draw) and one asynchronous EAGLE-3 run on tests/golden/tiny_eagle3.npz.

  * eager (enforce_eager=True: every body runs on every step): the whole ordered trace -- function name, scalar arguments, shape and
    dtype of every tensor argument -- and the generated token ids;
  * graphs: the set of graph names each runner created, and the generated token ids (they differ from the eager ones under sampling:
    a capture's warm-up run advances the device RNG).

Token ids are only stored for runs whose two recordings agreed.  The recording is written by this file's own record mode on the GPU,

    python tests/test_launch_trace_gpu.py --record [--commit HASH]

from the tree whose behaviour is to be pinned, and is not re-recorded by a change that claims to leave behaviour alone."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "launch_trace.json")

pytestmark = pytest.mark.gpu

K, N_NEW = 3, 6
MODES = ("ar", "sync", "async")
SAMPLING = {
    "greedy": dict(temperature=0),
    "temp": dict(temperature=0.7),
    "temp_top_p": dict(temperature=0.7, top_p=0.9),
    "greedy_rep": dict(temperature=0, repetition_penalty=1.2),
    "temp_top_k_rep_bias": dict(temperature=0.7, top_k=5, repetition_penalty=1.2, logit_bias={3: 4.0}),
}
# name -> (mode, sampling setting, extra engine arguments)
SCENARIOS = {f"{m}-{s}": (m, s, {}) for m in MODES for s in SAMPLING}
SCENARIOS["async-temp-sampler_x"] = ("async", "temp", dict(sampler_x=0.8))
SCENARIOS["eagle-greedy"] = ("eagle", "greedy", {})
ENGINE_KW = dict(max_num_seqs=2, max_model_len=512, max_num_batched_tokens=512, kvcache_block_size=16, num_kvcache_blocks=64,
                 num_draft_kvcache_blocks=64)


def _golden(name):
    from oracle.io import load_npz
    return load_npz(os.path.join(ROOT, "tests", "golden", name + ".npz"))


def make_engine(mode: str, extra: dict, eager: bool):
    """(engine, the two prompts).  The second prompt is the first one reversed and shortened: two sequences of different lengths."""
    from ssd_amd.engine.llm_engine import LLMEngine, hip_runner_factory
    from ssd_amd.model_config import ModelConfig
    if mode == "eagle":
        from tests.util import eagle_models_from_golden
        g = _golden("tiny_eagle3")
        tcfg, tw, dcfg, dw, taps, _, _ = eagle_models_from_golden(g)
    else:
        g = _golden("tiny_llama")
        ci, cf = g["cfg_i"].tolist(), g["cfg_f"].tolist()
        tcfg = dcfg = ModelConfig("llama", ci[0], ci[1], ci[2], ci[3], ci[4], ci[5], ci[6], cf[0], cf[1], ci[7], False)
        tw = dw = {k[2:]: v for k, v in g.items() if k.startswith("w.")}

    def factory(config, model_cfg, *, is_draft, topo, **kw):
        return hip_runner_factory(config, model_cfg, is_draft=is_draft, topo=topo, weight_source=iter((dw if is_draft else tw).items()), **kw)

    kw = dict(ENGINE_KW, hf_config=tcfg, runner_factory=factory, enforce_eager=eager, **extra)
    if mode != "ar":
        kw.update(draft="d", draft_hf_config=dcfg, speculate=True, speculate_k=K, jit_speculate=True)
    if mode in ("async", "eagle"):
        kw.update(draft_async=True, async_fan_out=3, inprocess_draft=True)
    if mode == "eagle":
        kw.update(use_eagle=True, eagle_layers=list(taps))
    prompt = g["prompt"].tolist()
    return LLMEngine("t", **kw), [prompt, prompt[::-1][:13]]


def describe(v) -> str:
    if isinstance(v, torch.Tensor):
        return f"{str(v.dtype).replace('torch.', '')}{list(v.shape)}"
    if v is None or isinstance(v, (bool, int, float)):
        return repr(v)
    if isinstance(v, (list, tuple)):
        return "(" + ",".join(describe(x) for x in v) + ")"
    return type(v).__name__


def install_recorder(setattr_, trace: list) -> None:
    """Wrap every public callable of the three op modules (setattr_ is monkeypatch.setattr: undone with the monkeypatch)."""
    from ssd_amd.hip import ops, filter_ops, penalty_ops
    for mod in (ops, filter_ops, penalty_ops):
        short = mod.__name__.rsplit(".", 1)[1]
        for name, fn in list(vars(mod).items()):
            if name.startswith("_") or not callable(fn) or isinstance(fn, type) or getattr(fn, "__module__", None) != mod.__name__:
                continue

            def wrapper(*a, _fn=fn, _tag=f"{short}.{name}", **kw):
                trace.append(_tag + "(" + ", ".join([describe(x) for x in a] + [f"{k}={describe(x)}" for k, x in sorted(kw.items())]) + ")")
                return _fn(*a, **kw)
            setattr_(mod, name, wrapper)


def run_scenario(name: str, eager: bool, setattr_=None) -> dict:
    """One engine, one generate.  eager: {"trace", "tokens"}; otherwise {"graphs", "tokens"}."""
    from ssd_amd.sampling_params import SamplingParams
    mode, sampling, extra = SCENARIOS[name]
    eng, prompts = make_engine(mode, extra, eager)
    trace = []
    if eager:
        install_recorder(setattr_, trace)
    out, _ = eng.generate(prompts, SamplingParams(max_new_tokens=N_NEW, ignore_eos=True, **SAMPLING[sampling]), use_tqdm=False)
    res = {"tokens": [o["token_ids"] for o in out]}
    if eager:
        res["trace"] = trace
    else:
        runners = {"target": eng.model_runner, "draft": eng.draft_runner}
        res["graphs"] = {who: sorted({k[0] for k in r.graphs}) for who, r in runners.items() if r is not None}
    eng.exit()
    return res


@pytest.fixture(scope="module")
def recorded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_eager_launch_trace_is_the_recorded_one(recorded, monkeypatch, name):
    want = recorded["scenarios"][name]
    got = run_scenario(name, True, monkeypatch.setattr)
    monkeypatch.undo()
    want_trace = [recorded["entries"][i] for i in want["trace"]]
    assert len(want_trace) > 20
    for i, (a, b) in enumerate(zip(got["trace"], want_trace)):
        assert a == b, f"{name}: launch {i} differs from the recording\n  got      {a}\n  recorded {b}\n  after    {got['trace'][max(0, i - 3):i]}"
    assert len(got["trace"]) == len(want_trace), f"{name}: {len(got['trace'])} launches, {len(want_trace)} recorded"
    assert all(len(t) == N_NEW for t in got["tokens"])
    if want["eager_tokens"] is not None:
        assert got["tokens"] == want["eager_tokens"]


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_graph_names_and_tokens_are_the_recorded_ones(recorded, name):
    want = recorded["scenarios"][name]
    got = run_scenario(name, False)
    assert got["graphs"] == want["graphs"]
    assert all(len(t) == N_NEW for t in got["tokens"])
    if want["graph_tokens"] is not None:
        assert got["tokens"] == want["graph_tokens"]


def record(commit: str) -> None:
    """Run every scenario twice in both forms and write the fixture; token ids are kept where the two recordings agree, and traces
    and graph names must agree."""
    entries, index, scenarios, unstable = [], {}, {}, []
    for name in SCENARIOS:
        runs = []
        for _ in range(2):
            with pytest.MonkeyPatch.context() as mp:
                e = run_scenario(name, True, mp.setattr)
            runs.append((e, run_scenario(name, False)))
        (e0, g0), (e1, g1) = runs
        assert e0["trace"] == e1["trace"], f"{name}: the two recordings of the eager trace differ"
        assert g0["graphs"] == g1["graphs"], f"{name}: the two recordings of the graph names differ"
        for what, a, b in (("eager", e0, e1), ("graph", g0, g1)):
            if a["tokens"] != b["tokens"]:
                unstable.append(f"{name} ({what})")
        for t in e0["trace"]:
            if t not in index:
                index[t] = len(entries)
                entries.append(t)
        scenarios[name] = {"trace": [index[t] for t in e0["trace"]],
                           "eager_tokens": e0["tokens"] if e0["tokens"] == e1["tokens"] else None,
                           "graphs": g0["graphs"],
                           "graph_tokens": g0["tokens"] if g0["tokens"] == g1["tokens"] else None}
        print(f"{name}: {len(e0['trace'])} launches, graphs {g0['graphs']}, tokens {e0['tokens']} / {g0['tokens']}", flush=True)
    out = os.environ.get("LAUNCH_TRACE_OUT", FIXTURE)
    with open(out, "w") as f:
        json.dump({"recorded_at": commit, "token_ids_unstable": unstable, "entries": entries, "scenarios": scenarios}, f,
                  separators=(",", ":"))
        f.write("\n")
    print(f"wrote {out}: {len(entries)} distinct entries, token ids that differed between the two recordings: {unstable or 'none'}")


if __name__ == "__main__":
    assert "--record" in sys.argv, "usage: python tests/test_launch_trace_gpu.py --record [--commit HASH]"
    record(sys.argv[sys.argv.index("--commit") + 1] if "--commit" in sys.argv else "unknown")
