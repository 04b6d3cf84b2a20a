"""The device build stages (csrc/ploc_gpu.cpp, reinsert_gpu.cpp, collapse_gpu.cpp) on the degenerate geometry of
tests/adversarial_scenes.py: exact ties of the merge areas, zero extents, duplicates, half-areas that are all 0 or +inf,
signed zeros - at the smallest sizes that reach those stages and their block edges.  Each must return the bytes its host
twin returns (tests/test_builder_adversarial.py holds the host side to a valid, shallow, correct tree), and the tree must
trace on the GPU like the oracle walks it."""
import numpy as np
import pytest

import adversarial_scenes as A

pytestmark = pytest.mark.gpu

W, H = 64, 48


def _params(trx, device, **fields):
    def build(verts, counts):
        lib = trx.load()
        assert lib.trx_set_build_device(device) == 0
        return trx.flat_build_params(verts, counts, trx.build_params(**fields))
    return build


def _preset_device(trx, device):
    return lambda verts, counts: trx.flat_build_preset_device(verts, counts, preset="medium_build", device=device)


def _whole_iterations(trx, device):
    def build(verts, counts):   # the binned-SAH preset path, its reinsertion in whole-iteration batches
        lib = trx.load()
        assert lib.trx_set_build_preset(b"medium_build") == 0
        assert lib.trx_set_build_reinsertion_batches(1) == 0
        assert lib.trx_set_build_reinsertion(0.05, 6) == 0
        assert lib.trx_set_build_device(device) == 0
        return trx.flat_build(verts, counts)
    return build


MODES = {
    "default": lambda trx, device: _params(trx, device),
    "sort128": lambda trx, device: _params(trx, device, sort_precision=128),
    "no_reinsertion": lambda trx, device: _params(trx, device, reinsertion_batch_ratio=0.0),
    "medium_preset": _preset_device,
    "whole_iterations": _whole_iterations,
}

_verts = {}


def _scene(case):
    if case not in _verts:
        v = A.FINITE[case]()
        v.setflags(write=False)
        _verts[case] = v
    return _verts[case]


def _restore(lib):
    lib.trx_set_build_device(-1)
    lib.trx_set_build_reinsertion_batches(0)
    lib.trx_set_build_preset(b"medium_build")


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", list(A.FINITE))
def test_device_build_equals_host_build_on_adversarial_geometry(trx, orc, case, mode):
    lib = trx.load()
    verts = _scene(case)
    n = verts.shape[0]
    counts = np.array([n], dtype=np.uint64)
    try:
        host = MODES[mode](trx, -1)(verts, counts)
        dev = MODES[mode](trx, 0)(verts, counts)
    finally:
        _restore(lib)
    # raw bytes, not float values: -0.0 == +0.0 would hide a box minimum that came out with the other sign
    assert host.nodes.shape == dev.nodes.shape and host.nodes.tobytes() == dev.nodes.tobytes(), (case, mode)
    assert host.tri_source.tobytes() == dev.tri_source.tobytes(), (case, mode)
    assert host.tri_verts.tobytes() == dev.tri_verts.tobytes(), (case, mode)
    osc = orc.Scene.from_flat(dev)
    assert osc.validate() == (0, "")
    eye, look, fov = A.camera_for(verts)
    view = trx.view_from_camera(eye, look, fov, W, H)
    want, st = osc.trace_primary(orc.view_from_bytes(view), W, H, sem=3)
    assert st.overflow == 0
    sc = trx.Scene(dev)
    try:
        got, _ = sc.trace_primary(view, W, H, sem=3)
    finally:
        sc.close()
    assert (got["prim"] == want["prim"]).all() and (got["t"].view(np.uint32) == want["t"].view(np.uint32)).all()


@pytest.mark.parametrize("case", list(A.NON_FINITE))
def test_non_finite_vertices_are_refused_with_a_build_device_set(trx, case):
    lib = trx.load()
    verts = A.NON_FINITE[case]()
    n = verts.shape[0]
    counts = np.array([n], dtype=np.uint64)
    halves = np.array([n // 2, n - n // 2], dtype=np.uint64)
    try:
        assert lib.trx_set_build_device(0) == 0
        for call in (lambda: trx.flat_build(verts, counts),
                     lambda: trx.flat_build_params(verts, counts, trx.build_params()),
                     lambda: trx.flat_build_preset_device(verts, counts, preset="medium_build", device=0),
                     lambda: trx.flat_build_instanced(verts, halves, [0, 1, 1], None)):
            with pytest.raises(trx.TrxError, match="finite") as e:
                call()
            assert e.value.code == trx._lib.TRX_ERR_INVALID
    finally:
        _restore(lib)
