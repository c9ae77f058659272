"""The long-prefill GEMM (csrc/gemm_pf.hip gemm_lm_kernel): ssd_gemm_pf at 128 < M <= 16384 rows -- a whole prompt in one launch
per matrix instead of a loop of 128-row chunks -- against the oracle's F.linear, its bounds (no unwritten output, nothing written
past M rows / N columns / ldy), its determinism, the engine that uses it, and a 2-layer real-architecture prefill of 1024 tokens."""
import dataclasses
import math
import random

import pytest
import torch

from oracle import ops as O
from oracle import layout as LY
from tests.util import assert_close_bf16, assert_stream_matches, seq_margins, truth_forward

BF = torch.bfloat16
SENTINEL = 0x7FA5          # a NaN pattern no kernel produces (f2bf quiets NaNs to 0x7FC0 | ...)


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssd_amd.hip import ops
    return ops


def gpu_frag(H, w_dev, mode=0):
    R, K = w_dev.shape
    out = torch.empty(H.frag_numel(R, K), dtype=BF, device="cuda")        # exactly ceil(R/16) row groups: nothing past them
    H.rows_to_frag(w_dev.contiguous(), out, R, K, mode=mode)
    return out


def operands(M, N, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(M, K, generator=g, device="cuda").to(BF)
    w = (torch.randn(N, K, generator=g, device="cuda") * 0.05).to(BF)
    b = torch.randn(N, generator=g, device="cuda").to(BF)
    w[3, :] = 0.5
    x[M - 1, : K // 2] = -1.0
    return x, w, b


def check_rows(M, N, K):
    """Rows checked against the CPU oracle: all of them for small problems, else the edges of every tile form (0, M-1, 127/128,
    255/256, ...) plus a random sample."""
    if M * N * K <= (1 << 31):
        return list(range(M))
    rows = {0, 1, 15, 16, 127, 128, 129, 255, 256, 257, 383, 384, 511, 512, M - 17, M - 16, M - 2, M - 1}
    rows |= set(random.Random(M + N + K).sample(range(M), 24))
    return sorted(r for r in rows if 0 <= r < M)


def run_rows(H, xf, wf, M, N, K, bias=None, extra_rows=3, ld_pad=64, splits=0, nt=0):
    ldy = N + ld_pad
    yb = torch.full(((M + extra_rows) * ldy,), SENTINEL, dtype=torch.int16, device="cuda")
    y = yb.view(BF).view(M + extra_rows, ldy)
    ws = torch.zeros(max(H.gemm_pf_workspace_bytes(M, N, K), 16 * M * N * 4 if splits > 1 else 4) // 4, dtype=torch.float32, device="cuda")
    H.gemm_pf(xf, wf, y, M, N, K, ldy, ws, bias=bias, splits=splits, nt=nt)
    torch.cuda.synchronize()
    raw = yb.view(M + extra_rows, ldy)
    assert bool((raw[M:] == SENTINEL).all()), "a row >= M was written"
    assert bool((raw[:M, N:] == SENTINEL).all()), "a column >= N (inside ldy) was written"
    out = y[:M, :N]
    assert bool(torch.isfinite(out.float()).all()), "an output element was left unwritten"
    return out.clone()


MS = [129, 255, 256, 300, 1000, 2048, 4100]
NKS = [(128, 128), (1280, 128), (10240, 128), (128, 8192), (1280, 8192), (10240, 8192)]


@pytest.mark.gpu
@pytest.mark.parametrize("N,K", NKS, ids=[f"N{n}-K{k}" for n, k in NKS])
@pytest.mark.parametrize("M", MS)
def test_long_prefill_gemm_vs_oracle(H, M, N, K):
    """Default dispatch, with and without bias: <= 1 ulp on at most 3 % of the elements (accumulation order), every output written,
    nothing past M rows / N columns touched, two runs bit-equal."""
    x, w, b = operands(M, N, K, seed=M * 7 + N + K)
    xf, wf = gpu_frag(H, x), gpu_frag(H, w)
    rows = check_rows(M, N, K)
    xc, wc, bc = x[rows].cpu(), w.cpu(), b.cpu()
    for bias in (None, b):
        y = run_rows(H, xf, wf, M, N, K, bias=bias)
        ref = O.linear(xc, wc, None if bias is None else bc)
        assert_close_bf16(y[rows].cpu(), ref, max_ulp=1, max_frac=0.03, rel_floor=2 ** -7, what=f"long prefill M={M} N={N} K={K}")
    y2 = run_rows(H, xf, wf, M, N, K, bias=b)
    assert torch.equal(y2.view(torch.int16), y.view(torch.int16)), "two runs differ"


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [(300, 1280, 1024), (1000, 2560, 512), (2048, 8192, 2048)])
def test_long_prefill_tile_forms_are_bit_identical_and_split_k_is_close(H, M, N, K):
    """The four tile forms (ssd_gemm_pf_cfg nt = 1..4) only change who computes a tile, never the K order: bit-identical.  A K
    split sums fp32 partials in a fixed order: close to the oracle and deterministic."""
    x, w, b = operands(M, N, K, seed=M + N + K)
    xf, wf = gpu_frag(H, x), gpu_frag(H, w)
    base = run_rows(H, xf, wf, M, N, K, bias=b, nt=1, splits=1)
    rows = check_rows(M, N, K)
    ref = O.linear(x[rows].cpu(), w.cpu(), b.cpu())
    assert_close_bf16(base[rows].cpu(), ref, max_ulp=1, max_frac=0.03, rel_floor=2 ** -7, what="form 1")
    for form in (2, 3, 4):
        y = run_rows(H, xf, wf, M, N, K, bias=b, nt=form, splits=1)
        assert torch.equal(y.view(torch.int16), base.view(torch.int16)), f"form {form} differs from form 1"
    for splits in (2, 4):
        y = run_rows(H, xf, wf, M, N, K, bias=b, nt=4, splits=splits)
        assert_close_bf16(y[rows].cpu(), ref, max_ulp=1, max_frac=0.03, rel_floor=2 ** -7, what=f"split {splits}")
        y2 = run_rows(H, xf, wf, M, N, K, bias=b, nt=4, splits=splits)
        assert torch.equal(y.view(torch.int16), y2.view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("M,I,K,splits", [(129, 256, 512, 0), (300, 640, 1024, 0), (1000, 512, 2048, 1), (257, 512, 1024, 2)])
def test_long_prefill_silu_epilogue(H, M, I, K, splits):
    """SSD_EPI_SILU_FRAG: silu(bf16 gate) * bf16 up, fragment-major for down_proj, every row < M of the output written."""
    x, w, b = operands(M, 2 * I, K, seed=M + I)
    wf = gpu_frag(H, w, mode=1)            # gate / up row groups interleaved
    xf = gpu_frag(H, x)
    ref = O.silu_mul(O.linear(x.cpu(), w.cpu()))
    act_f = torch.full((H.frag_numel(M, I),), float("nan"), dtype=BF, device="cuda")
    ws = torch.zeros(max(H.gemm_pf_workspace_bytes(M, 2 * I, K), 16 * M * 2 * I * 4 if splits > 1 else 4) // 4, dtype=torch.float32,
                     device="cuda")
    H.gemm_pf(xf, wf, act_f, M, 2 * I, K, 0, ws, epilogue=H.EPI_SILU_FRAG, splits=splits)
    act = LY.frag_to_rows_ref(act_f.cpu(), M, I)
    assert torch.isfinite(act.float()).all()
    assert_close_bf16(act, ref, max_ulp=2, max_frac=0.04, rel_floor=2 ** -7, what="long prefill gemm+silu")


@pytest.mark.gpu
def test_long_prefill_refuses_partials_and_bad_shapes(H):
    """PF_EPI_PARTIALS stays a one-chunk (M <= 128) epilogue; M > 16384 and ragged N / K are refused before any launch."""
    M, N, K = 256, 256, 256
    x, w, _ = operands(M, N, K, seed=5)
    xf, wf = gpu_frag(H, x), gpu_frag(H, w)
    ws = torch.zeros(4 * M * N, dtype=torch.float32, device="cuda")
    with pytest.raises(Exception):
        H.gemm_pf(xf, wf, None, M, N, K, N, ws, epilogue=H.PF_EPI_PARTIALS)
    y = torch.zeros(M, N, dtype=BF, device="cuda")
    for m, n, k in ((16385, N, K), (M, 200, K), (M, N, 200)):
        with pytest.raises(Exception):
            H.gemm_pf(xf, wf, y, m, n, k, n, ws)


REAL = [("70b.qkv", 10240, 8192, False), ("70b.o", 8192, 8192, False), ("70b.gate_up", 57344, 8192, True),
        ("70b.down", 8192, 28672, False), ("8b.gate_up", 28672, 4096, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("label,N,K,silu", REAL, ids=[r[0] for r in REAL])
def test_long_prefill_real_shapes_default_dispatch(H, label, N, K, silu):
    """70B TP = 1 qkv / o / gate_up + SiLU / down and 8B gate_up at M = 2048 through the default dispatch; the oracle on a subset
    of rows including 0, M-1 and the tile boundaries."""
    M = 2048
    x, w, _ = operands(M, N, K, seed=N + K)
    xf = gpu_frag(H, x)
    rows = [0, 1, 127, 128, 255, 256, 257, 511, 512, 1023, 1024, 1500, 2046, M - 1]
    wc = w.cpu()
    if silu:
        I = N // 2
        wf = gpu_frag(H, w, mode=1)
        act_f = torch.full((H.frag_numel(M, I),), float("nan"), dtype=BF, device="cuda")
        ws = torch.zeros(max(H.gemm_pf_workspace_bytes(M, N, K), 4) // 4, dtype=torch.float32, device="cuda")
        H.gemm_pf(xf, wf, act_f, M, N, K, 0, ws, epilogue=H.EPI_SILU_FRAG)
        rows_out = torch.empty(M, I, dtype=BF, device="cuda")
        H.frag_to_rows(act_f, rows_out, M, I)
        got = rows_out.cpu()
        assert torch.isfinite(got.float()).all()
        ref = O.silu_mul(O.linear(x[rows].cpu(), wc))
        assert_close_bf16(got[rows], ref, max_ulp=2, max_frac=0.04, rel_floor=2 ** -7, what=f"{label} M={M}")
    else:
        wf = gpu_frag(H, w)
        y = run_rows(H, xf, wf, M, N, K, extra_rows=1, ld_pad=0)
        assert_close_bf16(y[rows].cpu(), O.linear(x[rows].cpu(), wc), max_ulp=1, max_frac=0.03, rel_floor=2 ** -7, what=f"{label} M={M}")


@pytest.mark.gpu
def test_long_prompt_runs_one_gemm_per_linear_in_engine(H, monkeypatch):
    """A 600-token prompt batched with a 300-token one (900 prefill rows) on a tiny model: every linear of the prefill is ONE
    gemm_pf launch over all 900 rows -- including matrices far below the 128-row path's size floor -- and the greedy streams
    match the CPU oracle engine up to near-ties."""
    from oracle.runner import oracle_runner_factory
    from ssd_amd.engine.llm_engine import LLMEngine
    from ssd_amd.model_config import ModelConfig
    from ssd_amd.sampling_params import SamplingParams
    t = ModelConfig("llama", 256, 2, 4, 2, 64, 512, 512, 1e-5, 5e5, 1024, False)
    prompts = [[(13 * j + 5) % 512 for j in range(600)], [(7 * j + 1) % 512 for j in range(300)]]
    kw = dict(hf_config=t, max_num_seqs=2, max_model_len=1024, max_num_batched_tokens=1024, kvcache_block_size=16,
              num_kvcache_blocks=96, weights_std=0.1)
    sp = SamplingParams(temperature=0, max_new_tokens=10, ignore_eos=True)
    calls = []
    import ssd_amd.hip.ops as ops
    real = ops.gemm_pf
    monkeypatch.setattr(ops, "gemm_pf", lambda *a, **k: (calls.append(a[3]), real(*a, **k))[1])
    gpu_out, _ = LLMEngine("t", **kw).generate(prompts, sp, use_tqdm=False)
    cpu_eng = LLMEngine("t", runner_factory=oracle_runner_factory(), **kw)
    cpu_out, _ = cpu_eng.generate(prompts, sp, use_tqdm=False)
    # 2 layers x (qkv, o, gate_up, down), each once over the whole 900-row batch; never in 128-row chunks
    assert calls.count(900) == 8 and all(c == 900 for c in calls), calls[:16]
    for i, (a, b) in enumerate(zip(gpu_out, cpu_out)):
        n = assert_stream_matches(a["token_ids"], b["token_ids"], seq_margins(cpu_eng.model_runner.margin_log, i), len(prompts[i]),
                                  what=f"long prefill seq {i}")
        print("long-prefill engine: identical tokens", n, "of", len(b["token_ids"]))


@pytest.mark.gpu
def test_long_prefill_two_layer_8b_cut_vs_oracle_and_exact_arithmetic(H, monkeypatch):
    """HipDecoder.forward of a 1024-token prompt through a 2-layer cut of Llama-3.1-8B (vocabulary cut to 16384 to keep the CPU
    reference cheap): the last row's logits must be as close to exact (float64) arithmetic as the oracle pipeline's are
    (rms <= 1.25 x + 1e-3), with the same argmax outside near-ties, and the K / V rows written to the paged cache must match
    the oracle's."""
    from oracle.model import OracleModel, Ctx
    from ssd_amd import weights as W
    from ssd_amd.model import HipDecoder, AttnMeta
    from ssd_amd.model_config import PRESETS
    cfg = dataclasses.replace(PRESETS["llama-3.1-8b"], num_layers=2, vocab_size=16384)
    full = W.synthetic_state_dict(cfg, seed=4, std=0.02)
    P, bs = 1024, 256
    nblocks = P // bs
    dec = HipDecoder(cfg, max_tokens=P, max_seqs=1, max_blocks=nblocks, block_size=bs, max_model_len=2048, device=torch.device("cuda", 0))
    dec.load_weights(iter(full.items()))
    dec.alloc_kv(nblocks)
    orc = OracleModel(cfg, full, nblocks, bs)
    random.seed(2)
    prompt = [random.randint(0, cfg.vocab_size - 1) for _ in range(P)]
    table = [2, 0, 3, 1]
    bt = torch.tensor([table], dtype=torch.int32)
    slots = torch.tensor([table[p // bs] * bs + p % bs for p in range(P)], dtype=torch.int32)
    ids, pos = torch.tensor(prompt, dtype=torch.int64), torch.arange(P, dtype=torch.int64)
    cu = torch.tensor([0, P], dtype=torch.int32)
    ref_h = orc.forward(ids, pos, Ctx("prefill", slot_mapping=slots, cu_q=cu, cu_k=cu))
    ref_h = ref_h[0] if isinstance(ref_h, tuple) else ref_h
    ref = orc.compute_logits(ref_h[-1:]).double()
    calls = []
    real = H.gemm_pf
    monkeypatch.setattr(H, "gemm_pf", lambda *a, **k: (calls.append(a[3]), real(*a, **k))[1])
    meta = AttnMeta(H.MODE_CAUSAL, 1, P, slots.cuda(), torch.tensor([P], dtype=torch.int32).cuda(), bt.cuda(), cu_q=cu.cuda())
    dec.forward(ids.cuda(), pos.cuda(), P, meta)
    n = dec.compute_logits(P, gather=torch.tensor([P - 1], dtype=torch.int32).cuda(), rows=1)
    assert calls.count(P) == 8, calls
    got = dec.logits[:n].double().cpu()
    truth = truth_forward(cfg, full, prompt)[-1:]
    rms = lambda e: e.pow(2).mean(-1).sqrt()
    e_hip, e_ref = (got - truth).abs(), (ref - truth).abs()
    print(f"8B x 2 layers, 1024-token prefill, last row: |HIP-truth| max {e_hip.max():.4f} rms {rms(e_hip).mean():.5f} | "
          f"|oracle-truth| max {e_ref.max():.4f} rms {rms(e_ref).mean():.5f} | |HIP-oracle| max {(got - ref).abs().max():.4f}")
    assert torch.isfinite(got).all()
    assert bool((rms(e_hip) <= 1.25 * rms(e_ref) + 1e-3).all())
    top2 = ref.topk(2, dim=-1).values
    thr = torch.clamp(2 * (got - ref).abs().max(-1).values, min=0.0625)
    assert bool(((got.argmax(-1) == ref.argmax(-1)) | ((top2[:, 0] - top2[:, 1]) < thr)).all())
    # K / V rows of the last layer, every position (layer 1 already carries layer 0's propagated 1-ulp flips): the mean held to the
    # bar test_real_shapes_gpu.py holds its 40-row 2-layer cut to, the max to twice it -- 1024 rows x 8 heads x 128 are 25x the
    # samples (measured on MI355X: max 0.0625 / 0.0391, mean 0.0046 / 0.0044 against tol 0.0625)
    for which in (0, 1):
        ref_rows = torch.stack([orc.kv_cache[which, 1, table[p // bs], p % bs] for p in range(P)]).float()
        got_rows = dec.kv_cache[1, which][torch.tensor([table[p // bs] for p in range(P)]), :, torch.arange(P) % bs, :].cpu().float()
        tol = 2.0 ** (math.floor(math.log2(ref_rows.abs().max().item())) - 6)
        dkv = (got_rows - ref_rows).abs()
        print(f"   layer 1 {'KV'[which]} rows: |HIP-oracle| max {dkv.max():.4f} mean {dkv.mean():.6f} (tol {tol})")
        assert dkv.max().item() <= 2 * tol and dkv.mean().item() <= tol / 8


def test_long_prefill_workspace_query_and_validation_without_a_gpu():
    """ssd_gemm_pf_workspace_bytes at M > 128 answers SSD_OK with the largest need of any shorter prompt (so one buffer sized at
    max_tokens serves all), 0 where no K split is picked, and ssd_gemm_pf refuses bad long shapes before launching anything."""
    import ctypes
    from ssd_amd.hip.lib import load_library
    lib = load_library()

    def ws(M, N, K):
        out = ctypes.c_int64(-1)
        rc = lib.ssd_gemm_pf_workspace_bytes(M, N, K, ctypes.addressof(out))
        return rc, out.value

    for N, K in ((8192, 8192), (57344, 8192), (1280, 8192), (2048, 2048), (256, 512)):
        prev = 0
        for M in (129, 256, 300, 512, 1000, 2048, 4100, 8192, 16384):
            rc, b = ws(M, N, K)
            assert rc == 0 and b >= prev and b % 4 == 0, (N, K, M, rc, b)
            assert b >= max(ws(m, N, K)[1] for m in (129, 256, M) if m <= M), (N, K, M)
            prev = b
    assert ws(8192, 57344, 8192) == (0, 0)             # the big matrices never split K at long M: no workspace at all
    assert ws(16385, 8192, 8192)[0] < 0 and ws(300, 8192, 200)[0] < 0 and ws(300, 200, 8192)[0] < 0
    p = ctypes.c_void_p
    fn = lib.ssd_gemm_pf
    for M, N, K, epi in ((16385, 256, 256, 0), (300, 200, 256, 0), (300, 256, 200, 0), (300, 256, 256, 2), (300, 256, 256, 7)):
        rc = fn(p(0), p(0), p(0), p(0), M, N, K, N, epi, p(0), ctypes.c_int64(0), 0, p(0))
        assert rc < 0, (M, N, K, epi, rc)
    # a valid long shape with null operands is refused as an argument error, not launched
    assert fn(p(0), p(0), p(0), p(0), 300, 256, 256, 256, 0, p(0), ctypes.c_int64(0), 0, p(0)) < 0
