"""The zero-point W4A16 GEMM (csrc/gemm_w4a16.hip, ZP instantiations) at the edges of tests/test_hip_quant_edges.py: that file's case
table, harness, bars and test bodies, imported and run through one more per-format adapter -- K remainders and idle waves, every M
around the tile borders, ragged tiles per workgroup, sentinel-guarded outputs, poisoned x padding, SILU_FRAG + bias, the _cfg
refusals -- for every zero-point instantiation (`kernels` below restates W4<true>::FORMS)."""
from __future__ import annotations

import pytest
import torch

from tests import test_hip_quant_edges as E
from tests.test_hip_mxfp4 import dev  # noqa: F401  (the fixture)
from tests.test_hip_w4zp import _codes, _exact, _frag

gpu = pytest.mark.gpu


class _W4Z:
    """unsigned int4 codes, one bf16 scale and one zero point in 0..15 per row and 128 columns; a unit is 128 columns.  The kernels
    are the symmetric ones' decompositions, except that at 3-4 token tiles and two row groups x is loaded per group."""
    name, kunit = "w4a16_zp", 128
    kernels = dict(E._W4_KERNELS)
    kernels[(4, 2, False)] = (1, False)

    def rows(self, N, K, dev, seed):
        return _codes(N, K, dev, seed)                          # u, s, z, packed

    def exact(self, rows):
        """s[n, k / 128] * (u[n, k] - z[n, k / 128]), u decoded from the packed words the kernel is given."""
        u, s, z, packed = rows
        shifts = torch.arange(0, 32, 4, dtype=torch.int64, device=packed.device)
        codes = ((packed.to(torch.int64)[..., None] >> shifts) & 15).reshape(u.shape)
        assert torch.equal(codes, u.to(torch.int64))
        assert int(z.min()) == 0 and int(z.max()) == 15 and int(u.min()) == 0 and int(u.max()) == 15
        return _exact(u, s, z)

    def frag(self, rows, N, K, dev, rmap):
        return _frag(rows[3], rows[1], rows[2], N, K, dev, rmap)

    def gemm(self, xf, w, y, M, N, K, ldy, epilogue, bias, cfg):
        from ssd_amd.hip import w4zp_ops as W4Z
        W4Z.gemm_w4a16_zp(xf, w[0], w[1], w[2], y, M, N, K, ldy, epilogue=epilogue, bias=bias, cfg=cfg)


ZP = _W4Z()


def test_case_table_covers_every_zero_point_kernel_and_every_edge():
    assert ZP.name not in E.FORMATS and set(ZP.kernels) == set(E._W4_KERNELS)
    E.test_case_table_covers_every_kernel_and_every_edge(ZP)


@gpu
def test_m_sweep(dev):
    E.test_m_sweep(dev, ZP)


@gpu
def test_k_sweep(dev):
    E.test_k_sweep(dev, ZP)


@gpu
def test_silu_frag_with_bias_in_packed_order(dev):
    E.test_silu_frag_with_bias_in_packed_order(dev, ZP)


@gpu
def test_tile_sweep_bit_identical_across_tiles_per_workgroup(dev):
    E.test_tile_sweep_bit_identical_across_tiles_per_workgroup(dev, ZP)


@gpu
def test_cfg_refusals_return_an_error_and_launch_nothing(dev):
    E.test_cfg_refusals_return_an_error_and_launch_nothing(dev, ZP)


@gpu
def test_bounds_rows_past_m_columns_past_n_and_the_fragment_tail_stay_untouched(dev):
    E.test_bounds_rows_past_m_columns_past_n_and_the_fragment_tail_stay_untouched(dev, ZP)


@gpu
def test_poisoned_x_padding_rows_never_reach_a_real_output(dev):
    E.test_poisoned_x_padding_rows_never_reach_a_real_output(dev, ZP)
