"""The block-scaled FP8 GEMM (csrc/gemm_fp8b.hip) at the edges of tests/test_hip_quant_edges.py: that file's case table, harness, bars
and test bodies, imported and run through one more per-format adapter -- K remainders and idle waves (odd unit counts end in half a
scale block), every M around the tile borders, ragged tiles per workgroup, sentinel-guarded outputs, poisoned x padding, SILU_FRAG +
bias, the _cfg refusals -- for every instantiation (`kernels` below restates Fp8B::FORMS).

The scale table is group-granular, [N / 16][ceil(K / 128)] with every entry independently random and not a power of two
(tests/test_hip_fp8b.py::_codes): the table's shapes are 1 to 36 row groups and 1 to 22 units, so a kernel that indexed the table by
the unit instead of the block, by the row group without the tile's offset, or that did not advance it with the tile, reads a
different scale and fails."""
from __future__ import annotations

import pytest
import torch

from tests import test_hip_quant_edges as E
from tests.test_hip_mxfp4 import dev  # noqa: F401  (the fixture)
from tests.test_hip_fp8b import _codes, _exact, _frag

gpu = pytest.mark.gpu


class _Fp8B:
    """e4m3fn codes [N, K] (uint8) and one fp32 scale per 16-row group and 128 columns; a unit is 64 columns.  The kernels are fp8's
    decompositions, except that at 5-8 token tiles and two row groups x is loaded per unit."""
    name, kunit = "fp8b", 64
    kernels = dict(E.FORMATS["fp8"].kernels)
    kernels[(8, 2, False)] = (1, False)

    def rows(self, N, K, dev, seed):
        return _codes(N, K, dev, seed)                          # codes, group table in source row order

    def exact(self, rows):
        """s[n / 16, k / 128] * e4m3(code[n, k]) in float64."""
        codes, table = rows
        assert tuple(table.shape) == (codes.shape[0] // 16, -(-codes.shape[1] // 128))
        frac = torch.frexp(table)[0]
        assert bool((frac != 0.5).all()), "a power-of-two scale"
        return _exact(codes, table)

    def frag(self, rows, N, K, dev, rmap):
        return _frag(rows[0], rows[1], N, K, dev, rmap)

    def gemm(self, xf, w, y, M, N, K, ldy, epilogue, bias, cfg):
        from ssd_amd.hip import fp8b_ops as F8B
        F8B.gemm_fp8b(xf, w[0], w[1], y, M, N, K, ldy, epilogue=epilogue, bias=bias, cfg=cfg)


F8B = _Fp8B()


def test_case_table_covers_every_block_scaled_kernel_and_every_edge():
    assert F8B.name not in E.FORMATS and set(F8B.kernels) == set(E.FORMATS["fp8"].kernels)
    E.test_case_table_covers_every_kernel_and_every_edge(F8B)
    # odd unit counts (a half last block) and several scale blocks and row groups are in the K and tile sweeps
    t = E.table(F8B)
    assert any((c.K // 64) % 2 and c.K // 64 > 2 for c in t if c.sweep == "k")
    assert any(c.N // 16 > c.nt > 0 and c.tpw > 1 for c in t if c.sweep == "tile")


@gpu
def test_m_sweep(dev):
    E.test_m_sweep(dev, F8B)


@gpu
def test_k_sweep(dev):
    E.test_k_sweep(dev, F8B)


@gpu
def test_silu_frag_with_bias_in_packed_order(dev):
    E.test_silu_frag_with_bias_in_packed_order(dev, F8B)


@gpu
def test_tile_sweep_bit_identical_across_tiles_per_workgroup(dev):
    E.test_tile_sweep_bit_identical_across_tiles_per_workgroup(dev, F8B)


@gpu
def test_cfg_refusals_return_an_error_and_launch_nothing(dev):
    E.test_cfg_refusals_return_an_error_and_launch_nothing(dev, F8B)


@gpu
def test_bounds_rows_past_m_columns_past_n_and_the_fragment_tail_stay_untouched(dev):
    E.test_bounds_rows_past_m_columns_past_n_and_the_fragment_tail_stay_untouched(dev, F8B)


@gpu
def test_poisoned_x_padding_rows_never_reach_a_real_output(dev):
    E.test_poisoned_x_padding_rows_never_reach_a_real_output(dev, F8B)
