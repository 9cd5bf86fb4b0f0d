"""What the many-model routes share, on the host alone: _engine.next_chunk against a transcription of
the loop it was lifted from, _many.per_member on the cases of both modules' broadcast tests, and
_many.pack_members / unpack_members on CPU tensors."""
import numpy as np
import pytest
import torch


def inline_chunk(stops, max_iters, ii, sync_every, breaks):
    """The chunk logic as run_resident_many carried it inline (run_linear_many: the same with no breaks)."""
    left = np.where(stops == 0, max_iters - ii, 0)
    if not (left > 0).any():
        return None
    n = min([int(sync_every), int(left.max())] + [b - ii for b in breaks if b > ii])
    return n, np.clip(left, 0, n)


def walk(max_iter, sync_every=64, breaks=(), stop_at=None):
    """Runs the chunk loop on the host: [(ii, n, n_iters per member)].  stop_at: {member: loop index at
    which it stops on its plateau} (the stop shows in the stop array of the chunk that reaches it)."""
    from tensor_regression_amd import _engine
    max_iters = np.array([max(int(m), 0) for m in max_iter], dtype=np.int64)
    stops = np.zeros(len(max_iter), dtype=np.int32)
    ii, out = 0, []
    while True:
        got = _engine.next_chunk(stops, max_iters, ii, sync_every, breaks)
        want = inline_chunk(stops, max_iters, ii, sync_every, breaks)
        if want is None:
            assert got is None
            return out
        assert got[0] == want[0] and np.array_equal(got[1], want[1])
        n, iters = got
        assert 1 <= n <= sync_every and iters.max() == n and (iters >= 0).all()
        out.append((ii, n, iters.tolist()))
        for j, at in (stop_at or {}).items():
            if stops[j] == 0 and ii < at <= ii + n:
                stops[j] = at
        ii += n
        assert len(out) < 1000


def test_next_chunk_cases():
    assert walk([5, 5, 5]) == [(0, 5, [5, 5, 5])]                                   # all members equal
    assert walk([0, 130]) == [(0, 64, [0, 64]), (64, 64, [0, 64]), (128, 2, [0, 2])]  # one member with max_iter 0
    assert walk([-3, 2]) == [(0, 2, [0, 2])]
    # member 1 stops on its plateau in the first chunk: nothing for it from then on
    assert walk([100, 100, 70], stop_at={1: 40}) == [(0, 64, [64, 64, 64]), (64, 36, [36, 0, 6])]
    assert walk([65]) == [(0, 64, [64]), (64, 1, [1])]                              # 64 then 1
    assert walk([65, 3]) == [(0, 64, [64, 3]), (64, 1, [1, 0])]
    # breaks at 3 and 64 cut the first chunk to 3 and the next at 64
    assert walk([100, 10], breaks=[3, 64]) == [(0, 3, [3, 3]), (3, 61, [61, 7]), (64, 36, [36, 0])]
    assert walk([3, 2], sync_every=1) == [(0, 1, [1, 1]), (1, 1, [1, 1]), (2, 1, [1, 0])]
    assert walk([0, 0]) == [] and walk([]) == []                                    # every member done


def test_next_chunk_is_none_when_all_stopped_or_spent():
    from tensor_regression_amd import _engine
    mx = np.array([10, 20], dtype=np.int64)
    assert _engine.next_chunk(np.array([4, -7], dtype=np.int32), mx, 7, 64, ()) is None
    assert _engine.next_chunk(np.zeros(2, dtype=np.int32), mx, 20, 64, ()) is None
    n, iters = _engine.next_chunk(np.array([0, 9], dtype=np.int32), mx, 9, 64, [5, 9])  # breaks behind ii do not cut
    assert n == 1 and iters.tolist() == [1, 0]


def test_per_member_shared():
    from tensor_regression_amd import _many
    from tensor_regression_amd import multinomial_tensor_regression_hierarchical as H
    from tensor_regression_amd import standard_tensor_regression as S
    per = _many.per_member
    ak = {"lr": 0.1}
    assert per("lambda_L2", 0.01, 3) == [0.01] * 3
    assert per("max_iter", [1, 2, 3], 3) == [1, 2, 3]
    assert per("tol", (0.0, 1e-5), 2) == [0.0, 1e-5]
    assert per("Adam_kwargs", ak, 2) == [ak, ak]
    assert per("Adam_kwargs", [ak, None], 2) == [ak, None]
    for name, value, M in (("lambda_L2", [0.1, 0.2], 3), ("Adam_kwargs", [ak], 2), ("patience", [], 1)):
        with pytest.raises(ValueError, match="one value per model"):
            per(name, value, M)
    # a value that is itself a sequence: one for all, or a list of one per model
    one = [0.1, [(0, 0.1), (3, 0.2)], 0.3]
    sched = H._one_schedule
    assert per("group_lr", None, 2, sched) == [None, None]
    assert per("group_lr", one, 2, sched) == [one, one]
    assert per("group_lr", one, 3, sched) == [one] * 3
    assert per("group_lr", [0.1, 0.2, 0.3], 3, sched) == [[0.1, 0.2, 0.3]] * 3
    assert per("group_lr", [None, one, None], 3, sched) == [None, one, None]
    assert per("group_lr", [one, [0.1, 0.2, 0.3], one], 3, sched) == [one, [0.1, 0.2, 0.3], one]
    assert per("group_lr", [one, None], 2, sched) == [one, None]
    for value, M in (([None, None], 3), ([one, one], 3)):
        with pytest.raises(ValueError, match="one value per model"):
            per("group_lr", value, M, sched)
    # both modules' _per_member are this function
    assert S._per_member("tol", (0.0, 1e-5), 2) == [0.0, 1e-5]
    assert H._per_member("group_lr", one, 2) == [one, one] and H._per_member("tol", (0.0, 1e-5), 2) == [0.0, 1e-5]


def _members(style, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for I0, I1, R in ((3, 4, 2), (8, 5, 3), (1, 7, 1)):  # unequal sizes
        if style == "linear":  # factor, factor, 1-element bias
            out.append([torch.randn(I0, R, generator=g), torch.randn(I1, R, generator=g), torch.randn(1, generator=g)])
        else:  # three factors
            out.append([torch.randn(I0, R, generator=g), torch.randn(I1, R, generator=g),
                        torch.randn(4, R, generator=g)])
    return out


@pytest.mark.parametrize("style", ["linear", "multinomial"])
def test_pack_unpack_round_trip(style):
    from tensor_regression_amd import _many
    params = _members(style, 0)
    arena, offsets, slices = _many.pack_members(params, "cpu")
    flat = [t for p in params for t in p]
    sizes = [t.numel() for t in flat]
    assert arena.dtype == torch.float32 and arena.numel() == sum(sizes)
    assert offsets == [int(v) for v in np.cumsum([0] + sizes[:-1])]
    assert len(slices) == 3 and [s.numel() for s in slices] == [sum(t.numel() for t in p) for p in params]
    for s, p in zip(slices, params):
        assert torch.equal(s, torch.cat([t.reshape(-1) for t in p]))
    # a slice is a view of the arena: what a fit writes there is what unpack copies back
    assert slices[1].data_ptr() == arena.data_ptr() + 4 * offsets[3]
    want = [t.clone() for t in flat]
    arena.mul_(2.0)
    dsts = [[torch.zeros_like(t) for t in p] for p in params]
    _many.unpack_members(arena, offsets, dsts)
    for d, w in zip([t for p in dsts for t in p], want):
        assert d.shape == w.shape and torch.equal(d, 2.0 * w)
