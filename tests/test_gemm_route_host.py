"""Which GEMM shapes take the 256 x 256 tile kernel: cpx_gemm_uses_big_tile pinned against the rule restated here.  Host only:
the query is plain arithmetic inside the library (the same function the launcher asks), so the library answers without a device.

The block driver decides by this answer whether the residual GEMMs emit the LayerNorm row statistics themselves, and the GPU tests
assert the route of every case by it; here both sides of every clause of the rule are checked.
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from classpose_amd import _lib, ops  # noqa: E402


def rule(M, N, K, epi):
    """big tile iff: not the f32 epilogue; whole 256^2 tiles; at least two K tiles of 64; an even number of them unless the
    epilogue is the positional one; at least 256 tiles (one per CU)"""
    return int(epi != "f32" and M % 256 == 0 and N % 256 == 0 and K >= 128 and ((K // 64) % 2 == 0 or epi == "pos")
               and (M // 256) * (N // 256) >= 256)


CASES = [
    (16384, 1024, 1024, "resid", 1),    # 256 tiles
    (16128, 1024, 1024, "resid", 0),    # 252 tiles
    (16384, 1024, 64, "resid", 0),
    (16384, 1024, 128, "resid", 1),
    (16384, 1024, 192, "pos", 1),       # three K tiles: the positional epilogue only
    (16384, 1024, 192, "bf16", 0),
    (16384, 1152, 1024, "resid", 0),    # N is no multiple of 256
    (16512, 1024, 1024, "resid", 0),    # M is no multiple of 256
    (16384, 1024, 1024, "f32", 0),
]
ENGINE_32 = [(32 * 1024, 3072, 1024, "qkv"), (32 * 1024, 1024, 1024, "resid"), (32 * 1024, 4096, 1024, "gelu"), (32 * 1024, 1024, 4096, "resid")]


@pytest.mark.parametrize("M,N,K,epi,expected", CASES)
def test_both_sides_of_every_clause(M, N, K, epi, expected):
    assert rule(M, N, K, epi) == expected
    assert _lib.lib().cpx_gemm_uses_big_tile(M, N, K, ops.EPI[epi]) == expected


@pytest.mark.parametrize("M,N,K,epi", ENGINE_32)
def test_engine_shapes_at_32_subtiles_take_the_big_tile(M, N, K, epi):
    assert rule(M, N, K, epi) == 1
    assert _lib.lib().cpx_gemm_uses_big_tile(M, N, K, ops.EPI[epi]) == 1


def test_library_follows_the_rule_on_a_grid_of_shapes():
    L = _lib.lib()
    for epi in ops.EPI:
        for M in (256, 16128, 16384, 16512, 32768):
            for N in (128, 1024, 1152, 3072):
                for K in (64, 128, 192, 256, 1024):
                    assert L.cpx_gemm_uses_big_tile(M, N, K, ops.EPI[epi]) == rule(M, N, K, epi), (M, N, K, epi)
