"""CPU: the helpers every entry point shares (vexautonomousplanner_amd/_call.py), with torch.device("cpu") standing in
for the device: nothing here reaches libvap.so."""
import ctypes as C

import numpy as np
import pytest
import torch

from vexautonomousplanner_amd import _call

CPU = torch.device("cpu")
SHAPES = {"a": ((3, 2), torch.float64), "n": ((3,), torch.int32)}


def test_buffers_keeps_a_matching_entry_and_leaves_other_keys_alone():
    a, n, other = torch.zeros((3, 2), dtype=torch.float64), torch.zeros(3, dtype=torch.int32), object()
    out = {"a": a, "n": n, "other": other}
    res = _call.buffers(out, SHAPES, CPU)
    assert res is out and set(out) == {"a", "n", "other"}
    assert out["a"] is a and out["n"] is n and out["other"] is other


@pytest.mark.parametrize("wrong", [
    torch.zeros((2, 2), dtype=torch.float64),                 # shape
    torch.zeros((3, 2), dtype=torch.float32),                 # dtype
    torch.zeros((3, 2), dtype=torch.float64, device="meta"),  # device
    torch.zeros((2, 3), dtype=torch.float64).t(),             # contiguity: (3, 2) with strides (1, 3)
], ids=["shape", "dtype", "device", "contiguity"])
def test_buffers_replaces_a_mismatch(wrong):
    n = torch.zeros(3, dtype=torch.int32)
    out = {"a": wrong, "n": n}
    res = _call.buffers(out, SHAPES, CPU)
    assert res is out and out["n"] is n and out["a"] is not wrong
    t = out["a"]
    assert tuple(t.shape) == (3, 2) and t.dtype == torch.float64 and t.device == CPU and t.is_contiguous()


def test_buffers_without_out_gives_a_new_dict():
    res = _call.buffers(None, SHAPES, CPU)
    assert set(res) == {"a", "n"}
    for k, (shp, dt) in SHAPES.items():
        assert tuple(res[k].shape) == shp and res[k].dtype == dt and res[k].device == CPU and res[k].is_contiguous()
    assert _call.buffers(None, SHAPES, CPU) is not res


def test_ptr_and_dptr():
    assert _call.ptr(None) is None
    t = torch.arange(4, dtype=torch.float64)
    p = _call.ptr(t)
    assert isinstance(p, C.c_void_p) and p.value == t.data_ptr()
    assert _call.dptr(None) is None
    assert _call.dptr(np.zeros((0, 2))) is None
    a = np.array([1.5, -2.0])
    d = _call.dptr(a)
    assert C.addressof(d.contents) == a.ctypes.data and d[0] == 1.5 and d[1] == -2.0


@pytest.mark.parametrize("dtype, np_dtype", [(torch.float64, np.float64), (torch.int32, np.int32)])
def test_device_array(dtype, np_dtype):
    want = np.array([[1, 2, 3], [4, 5, 6]], dtype=np_dtype)
    other = np.float32 if np_dtype is np.float64 else np.int64
    strided = torch.tensor(want.T.copy()).t()                  # (2, 3) with strides (1, 2)
    assert not strided.is_contiguous()
    for given in ([[1, 2, 3], [4, 5, 6]], want.astype(other), np.asfortranarray(want), strided, strided.to(torch.float32)):
        t = _call.device_array(given, CPU, dtype)
        assert t.dtype == dtype and t.device == CPU and t.is_contiguous() and tuple(t.shape) == (2, 3)
        assert np.array_equal(t.numpy(), want)
    assert _call.device_array(None, CPU, dtype) is None
    fits = torch.tensor(want)
    assert _call.device_array(fits, CPU, dtype) is fits         # nothing to convert: used in place
