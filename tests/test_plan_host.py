"""The GEMM plan and its two surviving switches, host-only (cullavo_gemm_plan needs no GPU): the
default plans of the ViT fc1 product and the gate|up weight gradient (M-tail split on 288-row
tiles, the round split), cullavo_gemm_set_msplit turning both splits off and on again, and
cullavo_gemm_set_epilogue refusing every value retired with ABI 9 (it keeps its setting, and no
such value moves a plan any more)."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cullavo_amd import _lib  # noqa: E402

RETIRED_EPILOGUE = (2, 4, 8, 16, 32, 64, 128, 256, 512, 1 | 128, 1 | 512)


def plan(L, M, N, K, al=0, bl=0):
    g = ctypes.c_int64(0)
    return L.cullavo_gemm_plan(M, N, K, al, bl, ctypes.byref(g)), g.value


def test_round6_plan_defaults_and_switches():
    L = _lib.lib()
    prev_e = L.cullavo_gemm_set_epilogue(1)
    prev_m = L.cullavo_gemm_set_msplit(1)
    try:
        assert prev_e == 1 and prev_m == 1  # the defaults
        # ViT fc1 (M = 64 x 577): 288-row M-split, 128 M-tiles x 16 = 8 whole rounds
        assert plan(L, 36928, 4096, 1024) == (110, 2048)
        # the round split of the gate|up weight gradient: 5 whole rounds of 256x256 tiles
        assert plan(L, 22016, 4096, 8704, 1, 1) == (102, 1280)
        # a split never leaves a tail of <= 16 rows: 16 x 288 + 8 rows
        p, grid = plan(L, 16 * 288 + 8, 4096, 4096)
        if p >= 100:
            bm = {2: 256, 3: 192, 10: 288}[p - 100]
            assert 16 * 288 + 8 - grid // 16 * bm > 16
        # splits off: both products run whole on one tile; any non-zero value turns them on again
        assert L.cullavo_gemm_set_msplit(0) == 1
        assert plan(L, 36928, 4096, 1024)[0] < 100
        assert plan(L, 22016, 4096, 8704, 1, 1)[0] < 100
        assert L.cullavo_gemm_set_msplit(2) == 0
        assert L.cullavo_gemm_set_msplit(1) == 1
        assert plan(L, 36928, 4096, 1024) == (110, 2048)
        assert plan(L, 22016, 4096, 8704, 1, 1) == (102, 1280)
        # the epilogue values retired with ABI 9: the call returns the setting it leaves in place
        for setting in (1, 0):
            L.cullavo_gemm_set_epilogue(setting)
            for v in RETIRED_EPILOGUE:
                assert L.cullavo_gemm_set_epilogue(v) == setting, v
                assert plan(L, 36928, 4096, 1024) == (110, 2048), v
            assert L.cullavo_gemm_set_epilogue(1) == setting
    finally:
        L.cullavo_gemm_set_epilogue(prev_e)
        L.cullavo_gemm_set_msplit(prev_m)
