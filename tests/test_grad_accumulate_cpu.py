"""Gradient accumulation, the parts that need no GPU: both libraries export vpt_grad_accumulate_multi under the unchanged ABI number, the row
groups of micro_batches=K are distributed.shard_range's, and the micro-batches' totals are summed in fp64 in order, then rounded to fp32."""
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge
    ge.build()
    import vpt_amd  # noqa: F401
    from vpt_amd import _native
    return _native


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_both_libraries_export_the_kernel_under_abi_5(native, fmt):
    lib = native.load(fmt)
    assert hasattr(lib, "vpt_grad_accumulate_multi")
    assert lib.vpt_grad_accumulate_multi.argtypes == [ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_void_p]
    assert int(lib.vpt_abi_version()) == 5 == native.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "vpt_hip.h")).read()
    assert "int vpt_grad_accumulate_multi(const void* table, int ntensors, int64_t total_blocks, void* stream);" in hdr
    # the raw ctypes handle of the file on disk (not the typed, cached one): the symbol is in the shared object itself
    assert hasattr(ctypes.CDLL(native._LIB_PATHS[fmt]), "vpt_grad_accumulate_multi")


def test_null_table_is_refused_without_a_launch(native):
    """A null table with tensors to walk is an argument error (rc != 0, a message), not a launch."""
    lib = native.load("bf16")
    assert lib.vpt_grad_accumulate_multi(None, 3, 3, None) != 0
    assert b"vpt_grad_accumulate_multi" in lib.vpt_last_error()


def test_row_groups_are_shard_ranges(native):
    from vpt_amd.distributed import shard_range
    from vpt_amd.trainer_base import TrainerBase
    rows = TrainerBase.micro_batch_rows
    assert rows(4, 2) == [(0, 2), (2, 4)]
    assert rows(5, 2) == [(0, 3), (3, 5)]
    assert rows(3, 3) == [(0, 1), (1, 2), (2, 3)]
    assert rows(7, 1) == [(0, 7)]
    for b, k in ((4, 2), (5, 2), (3, 3), (64, 4), (9, 7)):
        got = rows(b, k)
        assert got == [shard_range(b, i, k) for i in range(k)]
        assert got[0][0] == 0 and got[-1][1] == b and all(a[1] == c[0] for a, c in zip(got, got[1:])) and all(hi > lo for lo, hi in got)
    for b, k in ((2, 3), (4, 0), (4, -1), (4, 1.5)):
        with pytest.raises(ValueError):
            rows(b, k)


def test_state_rows_and_their_concatenation_are_inverse(native):
    from vpt_amd.trainer_base import TrainerBase as T
    g = torch.Generator().manual_seed(0)
    state = [(None, (torch.randn(5, 4, 3, generator=g), torch.randn(5, 4, 3, generator=g))), (torch.rand(5, 1, 4, generator=g) > 0.5, (torch.randn(5, 0, 3), torch.randn(5, 0, 3)))]
    parts = [T._tree_rows(state, lo, hi) for lo, hi in T.micro_batch_rows(5, 2)]
    assert parts[0][0][0] is None and parts[0][0][1][0].shape == (3, 4, 3) and parts[1][1][0].shape == (2, 1, 4)
    back = T._tree_cat_rows(parts)
    assert back[0][0] is None and isinstance(back[0], tuple) and isinstance(back, list)
    assert torch.equal(back[0][1][0], state[0][1][0]) and torch.equal(back[0][1][1], state[0][1][1]) and torch.equal(back[1][0], state[1][0])
    assert back[1][1][0].shape == (5, 0, 3)


@pytest.mark.parametrize("n", [8, 16])
def test_totals_are_summed_in_fp64_in_order_then_rounded(native, n):
    """Pinned against numpy: ((t0 + t1) + t2) in float64, one rounding to float32 -- and an example where fp32 accumulation gives other bits."""
    from vpt_amd.trainer_base import TrainerBase
    rng = np.random.default_rng(n)
    parts = [(rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 6, n)).astype(np.float32) for _ in range(3)]
    parts[0][0], parts[1][0], parts[2][0] = np.float32(1.0), np.float32(2.0 ** -24), np.float32(2.0 ** -24)      # fp32: 1 + 2^-24 = 1 (ties to even), twice
    want = ((parts[0].astype(np.float64) + parts[1].astype(np.float64)) + parts[2].astype(np.float64)).astype(np.float32)
    got = TrainerBase.sum_totals([torch.from_numpy(p) for p in parts])
    assert got.dtype == torch.float32 and np.array_equal(got.numpy().view(np.int32), want.view(np.int32))
    f32 = (parts[0] + parts[1]) + parts[2]
    assert want[0] == np.float32(1.0 + 2.0 ** -23) and f32[0] == np.float32(1.0)
    one = TrainerBase.sum_totals([torch.from_numpy(parts[0])])
    assert np.array_equal(one.numpy().view(np.int32), parts[0].view(np.int32))
