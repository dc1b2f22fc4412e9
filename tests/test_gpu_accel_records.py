"""The traversal's acceleration data as data: every level of the padded min/max pyramid and of the node records, read
back through hf_get_node_level and held against the contract of tests/accel_ref.py (checks A-F), on the smallest shapes
that reach each branch of the build, on two strips that make hf_mip_top_kernel loop over a 4096-node depth, and after
every path that rebuilds the data.  Nothing is traced here.  tests/test_accel_ref.py shows that the checker can fail."""
import ctypes as C

import numpy as np
import pytest

import accel_ref as R

pytestmark = pytest.mark.gpu

_MARGINS = dict(contain=-np.inf, tight=-np.inf)      # the largest margins seen so far in this session (printed per test)


def _field(hf, h, s):
    import torch
    return hf.Heightfield(heightfield=torch.from_numpy(np.ascontiguousarray(h, np.float32)).cuda(), max_height=s)


def _read(shape, levels=None):
    out = {}
    for level in (levels or range(1, shape.num_levels() + 1)):
        rec, mm = shape.node_level(level)
        out[level] = (rec.numpy(), mm.numpy())
    return out


def _note(st, what):
    for k in _MARGINS:
        _MARGINS[k] = max(_MARGINS[k], st[k])
    print(f"{what}: (w - hi)/slack <= {st['contain']:.4g}, (hi - w_max)/eps_ref <= {st['tight']:.4g}; "
          f"so far {_MARGINS['contain']:.4g}, {_MARGINS['tight']:.4g}")


@pytest.mark.parametrize("W,H,kind,s", R.CASES)
def test_every_level_meets_the_contract(hf, W, H, kind, s):
    h = R.terrain(kind, W, H)
    shape = _field(hf, h, s)
    top = shape.num_levels()
    assert top == R.num_levels(W, H)
    data = _read(shape)
    for level, (rec, mm) in data.items():
        side = 1 << (top - level)
        assert rec.shape == (side, side, 12) and mm.shape == (side, side, 2)
    _note(R.check_all(h, s, W, H, data), f"{W}x{H} {kind} s={s}")
    # the global range that bbox (and the slab clip) read is the root slot
    bb = shape.bbox().numpy()
    root = data[top][1][0, 0]
    assert bb[0, 2].tobytes() == root[0].tobytes() and bb[1, 2].tobytes() == root[1].tobytes()


@pytest.mark.parametrize("W,H", [(2050, 2), (2, 2050)])
def test_strips_whose_top_kernel_loops(hf, W, H):
    """top = 12: depth 6 has 4096 nodes and one 1024-thread workgroup builds it, four nodes a thread.  Levels 6..12 are
    what that kernel writes; 3..5 are read too (levels 1 and 2 of a 4096 x 4096 padding are 250 MB of records that the
    other shapes cover)."""
    s = 0.5
    h = R.terrain("rand", W, H)
    shape = _field(hf, h, s)
    try:
        assert shape.num_levels() == 12
        data = _read(shape, range(3, 13))
        assert data[6][0].shape == (64, 64, 12)
        _note(R.check_all(h, s, W, H, data, levels=range(3, 13)), f"{W}x{H} strip")
        bb = shape.bbox().numpy()
        assert bb[0, 2] == data[12][1][0, 0, 0] == np.float32(0.5) * h.min() and bb[1, 2] == data[12][1][0, 0, 1]
    finally:
        shape.__del__()       # 0.3 GB of device memory: hf_destroy now, not at collection


def test_level_out_of_range_is_refused(hf):
    shape = _field(hf, R.terrain("rand", 34, 33), 0.5)
    assert shape.num_levels() == 6
    for level in (0, 7, -1):
        with pytest.raises(hf.HfError) as e:
            shape.node_level(level)
        assert e.value.code == 1 and "hf_get_node_level" in str(e.value)
    side = C.c_uint32()
    lib = hf._capi.lib()
    assert lib.hf_get_node_level(shape._h, 2, None, None, C.byref(side)) == 0 and side.value == 16
    assert lib.hf_get_node_level(shape._h, 2, None, None, None) == 0
    # either output alone
    rec, mm = shape.node_level(2)
    mm2 = np.empty((16, 16, 2), np.float32)
    assert lib.hf_get_node_level(shape._h, 2, None, mm2.ctypes.data, None) == 0 and np.array_equal(mm2, mm.numpy())
    rec2 = np.empty((16, 16, 12), np.float32)
    assert lib.hf_get_node_level(shape._h, 2, rec2.ctypes.data, None, None) == 0
    assert rec2.tobytes() == rec.numpy().tobytes()


# ---- rebuilds: whatever path rebuilt the data, it is bitwise the data of a fresh handle on the same heights --------

def _same_as_fresh(hf, shape, h, s, what):
    import torch
    torch.cuda.synchronize()
    fresh = _read(_field(hf, h, s))
    got = _read(shape)
    assert sorted(got) == sorted(fresh)
    for level in got:
        for name, a, b in (("records", got[level][0], fresh[level][0]), ("pyramid", got[level][1], fresh[level][1])):
            bad = a.view(np.uint32) != b.view(np.uint32)
            assert not bad.any(), f"{what}: level {level} {name} differ from a fresh handle's at {R._first(bad)}: " \
                                  f"{a[R._first(bad)]!r} != {b[R._first(bad)]!r}"
    W, H = h.shape[1], h.shape[0]
    R.check_all(h, s, W, H, got)       # (and the fresh handle's data is the contract's, not merely the same)


REBUILD_SHAPES = [(100, 37), (34, 33)]


def _two_terrains(W, H):
    a, b = R.terrain("rand", W, H, seed=1), R.terrain("sine", W, H)
    assert not np.array_equal(a, b)
    return a, b


@pytest.mark.parametrize("W,H", REBUILD_SHAPES)
def test_rebuild_by_set_heights(hf, W, H):
    import torch
    a, b = _two_terrains(W, H)
    shape = _field(hf, a, 0.5)
    before = _read(shape)
    shape.heightfield = torch.from_numpy(b).cuda()
    shape.parameters_changed(["heightfield"])          # hf_set_heights
    _same_as_fresh(hf, shape, b, 0.5, "hf_set_heights")
    assert any(not np.array_equal(before[L][0], r) for L, (r, _) in _read(shape).items())


@pytest.mark.parametrize("W,H", REBUILD_SHAPES)
def test_rebuild_by_set_heights_host(hf, W, H):
    from hf_amd import _capi
    a, b = _two_terrains(W, H)
    shape = _field(hf, a, 0.5)
    _capi.check(_capi.lib().hf_set_heights_host(shape._h, b.ctypes.data, shape._stream()))
    _same_as_fresh(hf, shape, b, 0.5, "hf_set_heights_host")


@pytest.mark.parametrize("W,H", REBUILD_SHAPES)
def test_rebuild_by_adam_step(hf, W, H):
    import torch
    a, _ = _two_terrains(W, H)
    shape = _field(hf, a, 0.5)
    opt = hf.Adam(shape, lr=0.05)
    rng = np.random.default_rng(3)
    shape.heightfield.grad = torch.from_numpy(rng.normal(size=(H, W)).astype(np.float32)).cuda()
    opt.step()                                          # hf_adam_step
    after = shape.heightfield.detach().cpu().numpy()
    assert np.abs(after - a).max() > 0.04
    _same_as_fresh(hf, shape, after, 0.5, "hf_adam_step")


@pytest.mark.parametrize("W,H", REBUILD_SHAPES)
def test_rebuild_by_two_scheduled_adam_steps(hf, W, H):
    import torch
    from hf_amd import _capi
    lib = _capi.lib()
    a, _ = _two_terrains(W, H)
    shape = _field(hf, a, 0.5)
    heights = shape.heightfield.detach()
    rng = np.random.default_rng(4)
    grad = torch.from_numpy(rng.normal(size=(H, W)).astype(np.float32)).cuda()
    m, v = torch.zeros_like(grad), torch.zeros_like(grad)
    lr_t = torch.tensor([lib.hf_adam_lr_t(0.05, 0.9, 0.999, k + 1) for k in range(4)], device="cuda")
    ctr = torch.zeros(1, dtype=torch.int32, device="cuda")
    for _ in range(2):
        _capi.check(lib.hf_adam_step_scheduled(shape._h, heights.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(),
                                               lr_t.data_ptr(), ctr.data_ptr(), 0.9, 0.999, 1e-8, 0, shape._stream()))
    torch.cuda.synchronize()
    assert int(ctr[0]) == 2
    after = heights.cpu().numpy()
    assert np.abs(after - a).max() > 0.08
    _same_as_fresh(hf, shape, after, 0.5, "hf_adam_step_scheduled x 2")


@pytest.mark.parametrize("W,H", REBUILD_SHAPES)
def test_rebuild_by_a_replayed_captured_set_heights(hf, W, H):
    """hf_set_heights from a caller-owned buffer, captured once; the buffer's contents at REPLAY are what the data is
    built from (capture pattern of tests/test_graph_capture.py)"""
    import torch
    from hf_amd import _capi
    lib = _capi.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    a, b = _two_terrains(W, H)
    shape = _field(hf, a, 0.5)
    buf = torch.from_numpy(a).to(dev)

    def step(stream):
        _capi.check(lib.hf_set_heights(shape._h, buf.data_ptr(), stream))

    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        step(s.cuda_stream)                              # warm-up on a side stream, as torch asks before a capture
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    _same_as_fresh(hf, shape, a, 0.5, "before the replay")
    buf.copy_(torch.from_numpy(b))
    g.replay()
    torch.cuda.synchronize()                             # a replayed rebuild does not record `built` (hf.h)
    _same_as_fresh(hf, shape, b, 0.5, "replayed captured hf_set_heights")
    del g
    _capi.check(lib.hf_capture_reset(shape._h))
