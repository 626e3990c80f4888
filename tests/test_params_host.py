"""The parameter blocks of the build-defined entry points (decode, note, PSOLA, flux, pick, timing) through the package's one
helper: the defaults are the ones the C entry point writes, an unknown key is a TypeError, and a value reaches C as its field's
type — a float given for an integer field truncated."""
import ctypes as C

import pytest

KINDS = {"decode": "f0_decode_params_default", "note": "note_params_default", "psola": "psola_params_default",
         "flux": "onset_flux_params_default", "pick": "onset_pick_params_default", "timing": "timing_params_default"}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_defaults_are_what_c_writes_and_unknown_keys_are_refused(mxlib, kind):
    struct, fn = mxlib._PARAMS[kind]
    p = struct()
    getattr(mxlib._capi.lib(), fn)(C.byref(p))
    d = getattr(mxlib, KINDS[kind])()
    assert list(d) == [k for k, _ in struct._fields_]
    for k, _ in struct._fields_:
        assert d[k] == getattr(p, k), (kind, k)
    assert mxlib._params_arg(kind, {}) is None  # nothing given: NULL, the library's defaults
    assert bytes(mxlib._params_arg(kind, {}, never_null=True)._obj) == bytes(p)
    name, value = next(iter(d.items()))
    assert bytes(mxlib._params_arg(kind, {name: value})._obj) == bytes(p)
    with pytest.raises(TypeError):
        mxlib._params_arg(kind, {"no_such_field": 1})
    with pytest.raises(TypeError):
        mxlib._params_arg(kind, {name: value, "no_such_field": 1}, never_null=True)


def test_a_float_for_an_integer_field_is_truncated(mxlib):
    from test_f0_host import SR, _track
    arg = mxlib._params_arg
    assert bytes(arg("decode", dict(max_jump_cents=1200.0))._obj) == bytes(arg("decode", dict(max_jump_cents=1200))._obj)
    assert bytes(arg("decode", dict(max_jump_cents=1200.5))._obj) == bytes(arg("decode", dict(max_jump_cents=1200))._obj)
    assert bytes(arg("decode", dict(max_jump_cents=700.0))._obj) != bytes(arg("decode", dict(max_jump_cents=1200))._obj)
    assert bytes(arg("note", dict(min_frames=8.0), never_null=True)._obj) == bytes(arg("note", dict(min_frames=8), never_null=True)._obj)
    assert bytes(arg("flux", dict(lag=2.0))._obj) == bytes(arg("flux", dict(lag=2))._obj)
    assert bytes(arg("timing", dict(bpm=90))._obj) == bytes(arg("timing", dict(bpm=90.0))._obj)  # and an int for a double
    tr = _track([45.0] * 20 + [47.0] * 20)
    notes = mxlib.detect_notes(tr, SR, 256, min_frames=8)
    assert len(notes) == 2 and mxlib.detect_notes(tr, SR, 256, min_frames=8.0).tobytes() == notes.tobytes()
    with pytest.raises(TypeError):
        mxlib.detect_notes(tr, SR, 256, no_such_field=1)
