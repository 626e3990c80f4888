"""The candidate ladder and the Viterbi f0 decoder without a GPU: the reference's chunked form against its serial form, what
the decoder does to the GLITCH signal, the parameter checks of the decode entry points, and the kernels' resource usage."""
import ctypes as C

import numpy as np
import pytest

import f0_decode_ref as D
import yin_ref as Y
from emu_build import resource_usage

CHUNKS = (1, 2, 7, 16, 64)


@pytest.fixture(scope="module")
def glitch_ref():
    """(plain F0_DTYPE track, F x 4 candidates in the device's layout) of GLITCH, by the f64 reference; read-only."""
    w = D.glitch()
    recs, _ = Y.track(w, D.GLITCH_SR, D.GLITCH_HOP)
    cands, _, _ = D.ladder(w, D.GLITCH_SR, D.GLITCH_HOP)
    plain, c32 = D.plain_track(recs), D.to_f32(cands)
    assert len(plain) == 375
    plain.setflags(write=False)
    c32.setflags(write=False)
    return plain, c32


def test_chunked_reference_equals_serial_on_glitch(glitch_ref):
    plain, cands = glitch_ref
    state, out = D.decode(plain, cands)
    for c in CHUNKS:
        s2, o2 = D.decode_chunked(plain, cands, c)
        assert s2.tobytes() == state.tobytes() and o2.tobytes() == out.tobytes(), c


@pytest.mark.parametrize("seed,F,params", [
    (1, 200, None),
    (2, 131, dict(unvoiced_cost=0.0, jump_cost=0.0, switch_cost=0.0, max_jump_cents=0)),
    (3, 65, dict(unvoiced_cost=2.5, jump_cost=16.0, switch_cost=0.0, max_jump_cents=12000)),
    (4, 1, None),
])
def test_chunked_reference_equals_serial_on_random_tables(seed, F, params):
    rng = np.random.default_rng(seed)
    stretches = ((5, 9), (60, 130)) if F > 130 else ((0, 1),) if F == 1 else ((5, 9),)
    track, cands = D.random_table(rng, F, stretches=stretches)
    assert (cands["tau"][stretches[0][0]:stretches[0][1]] == 0).all() and (cands["tau"] > 0).any() == (F > 1)
    state, out = D.decode(track, cands, params)
    assert ((state == D.UNVOICED) | (cands["tau"][np.arange(F), np.minimum(state, 3)] > 0)).all()  # never an empty slot
    assert (state[stretches[0][0]:stretches[0][1]] == D.UNVOICED).all()
    for c in CHUNKS:
        s2, o2 = D.decode_chunked(track, cands, c, params)
        assert s2.tobytes() == state.tobytes() and o2.tobytes() == out.tobytes(), c


def test_glitch_in_the_reference(glitch_ref):
    plain, cands = glitch_ref
    _, out = D.decode(plain, cands)
    D.glitch_assertions(plain, out, "reference")
    # the ladder's consequence: a plain record under the threshold is one of the slots, bit for bit
    for f in np.nonzero(plain["aperiodicity"] < np.float32(0.15))[0]:
        k = np.nonzero(cands["tau"][f] == plain["tau"][f])[0]
        assert len(k) == 1 and cands["period"][f, k[0]] == plain["period"][f]
        assert cands["aperiodicity"][f, k[0]] == plain["aperiodicity"][f]


def test_decode_parameter_checks_need_no_device(mxlib):
    """A bad parameter is refused before anything touches a context or a device, by all three decode entry points."""
    from melonix_amd import _capi

    lib = _capi.lib()
    d = mxlib.f0_decode_params_default()
    assert (np.float32(d["unvoiced_cost"]), np.float32(d["jump_cost"]), np.float32(d["switch_cost"]), d["max_jump_cents"]) == \
        (np.float32(0.3), np.float32(0.1), np.float32(0.5), 1200)
    bad = [dict(unvoiced_cost=-0.1), dict(jump_cost=16.5), dict(switch_cost=float("nan")), dict(unvoiced_cost=float("inf")),
           dict(max_jump_cents=-1), dict(max_jump_cents=12001)]
    tr = np.zeros(4, mxlib.F0_DTYPE)
    cd = np.zeros((4, 4), mxlib.F0_CAND_DTYPE)
    out = np.full(4 * 16, 0x5A, np.uint8)
    for kw in bad:
        p = _capi.F0DecodeParams(*[dict(d, **kw)[k] for k, _ in _capi.F0DecodeParams._fields_])
        word = "max_jump_cents" if "max_jump_cents" in kw else "decode cost"
        for call in (lambda: lib.mx_f0_decode(None, tr.ctypes.data, cd.ctypes.data, 4, C.byref(p), out.ctypes.data, None),
                     lambda: lib.mx_f0_decode_dev(None, tr.ctypes.data, cd.ctypes.data, 4, C.byref(p), out.ctypes.data, None),
                     lambda: lib.mx_f0_track_decoded(None, None, 48000, 256, 0, 4, 55.0, 1760.0, 0.15, C.byref(p),
                                                     out.ctypes.data)):
            assert call() == _capi.MX_ERR_INVALID, kw
            assert word in lib.mx_last_error().decode(), (kw, lib.mx_last_error())
        assert (out == 0x5A).all()
    # good parameters get as far as the missing context
    ok = _capi.F0DecodeParams(16.0, 0.0, 16.0, 12000)
    assert lib.mx_f0_decode(None, tr.ctypes.data, cd.ctypes.data, 4, C.byref(ok), out.ctypes.data, None) == _capi.MX_ERR_INVALID
    assert "context" in lib.mx_last_error().decode()
    assert lib.mx_f0_decode_set_chunk(None, 4) == _capi.MX_ERR_INVALID


def test_f0_kernels_do_not_spill():
    """Both f0_yin instantiations and the five decode kernels are scratch-free."""
    names, scratch, vgprs, _ = resource_usage("f0_kernels.hip")
    assert sum("f0_yinILb0" in n for n in names) == 1 and sum("f0_yinILb1" in n for n in names) == 1, names
    assert not [(n, s) for n, s in zip(names, scratch) if s != 0] and max(vgprs) <= 256
    names, scratch, vgprs, _ = resource_usage("f0_decode.hip")
    for k in ("f0_dec_products", "f0_dec_starts", "f0_dec_walk", "f0_dec_ends", "f0_dec_path"):
        assert any(k in n for n in names), (k, names)
    assert not [(n, s) for n, s in zip(names, scratch) if s != 0] and max(vgprs) <= 256
