"""GPU: _call.time_rows, and the five entry points that take time-domain rows through it: each refuses the same malformed
rows and gives the same bits for host rows as for device rows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT = 0.01


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def straight_rows(B, n):
    """(B, n, 8) rows of robots driving along +x at 1 ft/s, route b starting at (-1 + 2 b, b)."""
    rows = np.zeros((B, n, 8))
    t = np.arange(n) * DT
    rows[:, :, 0] = t
    rows[:, :, 1] = t
    rows[:, :, 2] = 1.0
    rows[:, :, 6] = -1.0 + 2.0 * np.arange(B)[:, None] + t
    rows[:, :, 7] = np.arange(B)[:, None]
    return rows


def same(torch, a, b):
    """The same shape, type and bits."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float64:
        a, b = a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)
    return torch.equal(a, b)


# ---------------------------------------------------------------- time_rows

def test_time_rows_host_and_device_agree(torch_mod):
    torch = torch_mod
    from vexautonomousplanner_amd._call import time_rows
    dev = torch.device("cuda", 0)
    batch, one = straight_rows(3, 5), straight_rows(1, 5)[0]
    for counts in (np.array([5, 3, 0]), np.array([[5, 1], [3, 1], [0, 0]])):
        k = 1 if counts.ndim == 1 else 2
        got = [time_rows(batch, counts),
               time_rows(torch.as_tensor(batch, device=dev), torch.as_tensor(counts, device=dev)),
               time_rows(np.asfortranarray(batch), counts.tolist(), None, 0, "side A")]
        for r, c, single, d in got:
            assert not single and d == dev
            assert r.dtype == torch.float64 and r.device == dev and r.is_contiguous() and tuple(r.shape) == (3, 5, 8)
            assert c.dtype == torch.int32 and c.device == dev and c.is_contiguous() and tuple(c.shape) == (3, k)
            assert np.array_equal(r.cpu().numpy(), batch) and np.array_equal(c.cpu().numpy(), counts.reshape(3, k))
    given = torch.as_tensor(batch, device=dev)
    assert time_rows(given, np.array([5, 3, 0]))[0].data_ptr() == given.data_ptr()        # a device tensor is used in place
    for rows in (one, torch.as_tensor(one, device=dev)):
        r, c, single, d = time_rows(rows, None)
        assert single and d == dev and tuple(r.shape) == (1, 5, 8) and np.array_equal(r.cpu().numpy()[0], one)
        assert c.dtype == torch.int32 and c.is_contiguous() and c.cpu().tolist() == [[5]]


@pytest.mark.parametrize("what, pre", [(None, ""), ("side A", "side A: ")])
def test_time_rows_messages(torch_mod, what, pre):
    torch = torch_mod
    from vexautonomousplanner_amd._call import time_rows
    dev = torch.device("cuda", 0)
    batch = straight_rows(3, 5)

    def message(rows, counts, on=None):
        with pytest.raises(ValueError) as e:
            time_rows(rows, counts, on, 0, what)
        return str(e.value)

    assert message(batch, None) == pre + "counts is needed for a batch of rows"
    fp64_only = pre + "rows must be an fp64 tensor on a HIP device (or a host array)"
    assert message(torch.as_tensor(batch, device=dev).float(), [5, 5, 5]) == fp64_only
    assert message(torch.as_tensor(batch), [5, 5, 5]) == fp64_only                       # a tensor on the host
    assert message(batch[:, :, :7], [5, 5, 5]) == pre + "rows must be (B, capacity, 8) or (n, 8), got (3, 5, 7)"
    assert message(batch, [[5], [5]]) == pre + "counts must be (3, k) or (3,), got (2, 1)"
    assert message(torch.as_tensor(batch, device=dev), None, torch.device("cuda", 1)) == \
        pre + "rows are on cuda:0, the other side on cuda:1"
    with pytest.raises((ValueError, RuntimeError)):       # two counts do not reshape to (3, 1): torch's own error
        time_rows(batch, [5, 5], None, 0, what)


# ---------------------------------------------------------------- the five entry points

def _clearance(rows, counts):
    from vexautonomousplanner_amd import footprint as fp
    return fp.clearance(rows, counts, fp.rectangle(18, 18), fp.Scene(), per_row=True)


def _conflicts(rows, counts):
    from vexautonomousplanner_amd import footprint as fp
    return fp.conflicts(rows, counts, fp.rectangle(18, 18), rows, counts, pairs=True)


def _rollouts(rows, counts):
    from vexautonomousplanner_amd import tracking
    pert = np.array([tracking.NOMINAL, (0.05, -0.05, 0.02, 1.02, 0.98, 1.0, 0.05, 0.0)])
    return tracking.rollouts(rows, counts, tracking.Follower(settle_rows=3), pert, time_step=DT)


def _occupancy(rows, counts):
    from vexautonomousplanner_amd import footprint as fp
    from vexautonomousplanner_amd import plan
    return plan.occupancy(rows, counts, fp.rectangle(18, 18), fp.Scene(), 0.5, 0.75, min_clearance=True)


def _chain(rows, counts):
    from vexautonomousplanner_amd import timeline
    res = timeline.chain(rows, counts, np.array([[0, 1]], dtype=np.int32), dt=DT)
    written = int(res["counts"][0, 0].item())
    return {**res, "rows": res["rows"][:, :written]}            # the rows behind a routine's count are not written


@pytest.mark.parametrize("call", [_clearance, _conflicts, _rollouts, _occupancy, _chain],
                         ids=["clearance", "conflicts", "rollouts", "occupancy", "chain"])
def test_entry_points_take_the_same_rows(torch_mod, call):
    torch = torch_mod
    with pytest.raises(ValueError, match=r"rows must be \(B, capacity, 8\) or \(n, 8\), got \(2, 4, 7\)"):
        call(straight_rows(2, 4)[:, :, :7], np.array([4, 4]))
    rows, counts = straight_rows(2, 4), np.array([[4, 0], [3, 0]])
    dev = torch.device("cuda", 0)
    on_host = call(rows, counts)
    on_device = call(torch.as_tensor(rows, device=dev), torch.as_tensor(counts, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    assert set(on_host) == set(on_device) and len(on_host) >= 5
    for k in on_host:
        assert same(torch, on_host[k], on_device[k]), k
