"""Key, scale and tuning reference without a GPU (include/melonix_amd.h "Key, scale and tuning reference"): the chroma
kernel's per-thread arithmetic (csrc/chroma_core.h behind stft_core.h's transform) run on the CPU by tests/emu/chroma_emu.cpp
against tests/key_ref.py, inside the bound key_ref derives from the arithmetic; the window sums byte for byte; mx_key_from_chroma,
mx_key_from_notes and mx_correction_markers_tuned of the library against the reference field for field; the refusals; the
kernels' resources; the reference alone against the truth of the synthetic takes."""
import ctypes as C
import math

import numpy as np
import pytest

import bad_samples as B
import emu_build
import key_ref as K
import yin_ref as Y

SR = K.SR
TAKES = ["c_major", "a_minor", "c_major_446", "c_major_flat_vibrato"]
KEY_FIELDS = ("tonic", "mode", "scale_mask", "tuning_cents", "tuning_confidence", "correlation", "clarity")
# Share of a take's frames that the guard may leave out of the parity check (a condition on the reference alone): frames that
# straddle two notes hold partials near the relative floor.  The takes lose 10 to 13 %, eight notes at 44.1 kHz in the
# 200-4000 Hz band 14 of 44.  Two thirds of every signal must stay in.
GUARD_SHARE = 1.0 / 3.0
# |tuning - truth| on the synthetic takes: the reference's own worst is 0.61 cents (a_minor; the partials' offset from equal
# temperament), so +-2 cents leaves it more than three times its error.
TUNING_BOUND = 2.0


class Case:
    """A signal with its reference: records, magnitude rows, peak lists, band and parameters (read-only, computed once)."""

    def __init__(self, w, sr=SR, hop=2048, first=0, count=None, **params):
        self.w, self.sr, self.hop, self.first, self.params = w, sr, hop, first, dict(K.CHROMA_DEFAULTS, **params)
        self.kmin, self.kmax = K.band(sr, self.params["fmin"], self.params["fmax"])
        self.ref, self.mags, self.peaks = K.chroma(w, sr, hop, first, count, details=True, **params)  # frames first ..
        self.ref.setflags(write=False)


def check_records(got, case, what, first=0):
    """got: (count, 40) f32 records of frames first.. of the case.  Frames whose peak decisions the guard (on the reference alone:
    every decision further than 100 x the magnitude yardstick from flipping) does not cover are left out and counted; the others
    lie inside key_ref.record_bound, column for column.  -> (worst error / bound, frames left out)."""
    got = np.asarray(got, dtype=np.float64).reshape(-1, K.COLS)
    assert np.isfinite(got).all(), what
    worst, out = 0.0, 0
    for i in range(len(got)):
        f = first + i - case.first
        m, pk = case.mags[f], case.peaks[f]
        dm = K.MAG_REL * m.max() + K.MAG_ABS
        if m.max() == 0.0:
            assert not got[i].any(), (what, f)
            continue
        margin = K.decision_margin(m, case.kmin, case.kmax, float(np.float32(case.params["floor"])), float(np.float32(case.params["rel"])))
        bound = K.record_bound(m, pk) if margin > 100 * dm else None
        if bound is None:
            out += 1
            continue
        assert got[i][39] == case.ref[f][39], (what, f, got[i][39], case.ref[f][39])
        err = np.abs(got[i] - case.ref[f])
        ratio = (err[:39] / bound[:39]).max() if len(pk) else float(err.max() > 0)
        assert ratio <= 1.0, (what, f, int(np.argmax(err[:39] / bound[:39])), ratio)
        worst = max(worst, ratio)
    return worst, out


@pytest.fixture(scope="module")
def cases():
    out = {name: Case(w) for name, (w, _, _, _) in K.takes().items()}
    out["chord"] = Case(K.chord())
    out["c_major_44100"] = Case(K.melody(K.C_MAJOR[:8], sr=44100), sr=44100, fmin=200.0, fmax=4000.0)
    out["noise"] = Case(K.noise(seconds=0.5))
    return out


@pytest.fixture(scope="module")
def emu(mxlib):
    L = C.CDLL(emu_build.shared_object("chroma_emu", ["chroma_emu.cpp"],
                                       ["chroma_core.h", "stft_core.h", "pk_math.h", "stft_tables.h", "stft_consts.inc"]))
    L.emu_chroma.restype = C.c_long
    L.emu_chroma.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_long, C.c_long, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int,
                             C.c_void_p]
    L.emu_chroma_sum.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_void_p]

    class Emu:
        @staticmethod
        def chroma(case, first=0, count=None, run=8):
            w = np.ascontiguousarray(case.w, dtype=np.float32)
            count = len(case.ref) - first if count is None else count
            out = np.zeros((count, K.COLS), dtype=np.float32)
            L.emu_chroma(w.ctypes.data, len(w), case.sr, case.hop, first, count, case.kmin, case.kmax, case.params["floor"],
                         case.params["rel"], run, out.ctypes.data)
            return out

        @staticmethod
        def sum(rec, first, frames):
            rec = np.ascontiguousarray(rec, dtype=np.float32)
            out = np.zeros(K.COLS)
            L.emu_chroma_sum(rec.ctypes.data, first, frames, out.ctypes.data)
            return out

    return Emu


# ---- the kernel's arithmetic on the CPU ----
@pytest.mark.parametrize("name", TAKES + ["chord", "c_major_44100"])
def test_the_kernels_arithmetic_on_the_cpu(emu, cases, name):
    case = cases[name]
    got = emu.chroma(case)
    worst, left_out = check_records(got, case, name)
    print(f"{name}: {len(got)} frames, {left_out} left out by the guard, worst error / bound {worst:.4f}")
    assert left_out <= GUARD_SHARE * len(got), (name, left_out)
    assert worst <= 0.25, name  # the arithmetic sits well inside the bound: most of it is the magnitude yardstick's allowance
    if name in ("c_major", "chord"):  # the same bytes whatever the run length or the launch split
        for run in (1, 5, 32):
            assert emu.chroma(case, run=run).tobytes() == got.tobytes(), run
        first, count = (37, 50) if name == "c_major" else (17, 7)
        assert emu.chroma(case, first, count, run=7).tobytes() == got[first:first + count].tobytes()
        assert emu.chroma(case, 5, 1, run=32).tobytes() == got[5:6].tobytes()


def test_noise_silence_and_bad_samples_on_the_cpu(emu, cases):
    noise = cases["noise"]
    got = emu.chroma(noise)
    assert np.isfinite(got).all() and got[:, 39].max() > 100  # hundreds of peaks a frame: the list well past a tonal frame's
    assert emu.chroma(noise, run=3).tobytes() == got.tobytes()
    np.testing.assert_allclose(got[:, :36].sum(axis=1), got[:, 38], rtol=1e-5)  # the bin window is a partition of unity
    silent = Case(np.zeros(9000, dtype=np.float32))
    assert emu.chroma(silent).tobytes() == bytes(160 * len(silent.ref))
    for bad in (np.inf, -np.inf, np.nan):
        w = cases["chord"].w[:12000].copy()
        w[5000] = bad
        case = Case(w)
        got = emu.chroma(case)
        holds = np.array([h * 2048 - 2048 <= 5000 < h * 2048 + 2048 for h in range(len(got))])
        assert holds.any() and not got[holds].any() and got[~holds][:, 38].all()
        assert not case.ref[holds].any()
        check_records(got, case, f"sample {bad}")


@pytest.mark.parametrize("k", B.CHROMA_SCALES)
def test_levels_far_off_full_scale_on_the_cpu(emu, cases, k):
    """The `chord` take times 2^k from 2^-140 (subnormal samples) to 2^126: a record is never Inf or NaN; forty zeros below the
    absolute floor and where the band maximum overflows f32 (2^80 and above); at 2^20 and 2^60 the peak count is the clean
    take's and the weight the clean one times 2^k, byte for byte, and the other columns lie inside key_ref's bound on the scaled
    take (tests/bad_samples.check_scaled_chroma says why they are not exact); 2^66 inside the bound as well."""
    clean = emu.chroma(cases["chord"])
    case = Case(B.scaled(cases["chord"].w, k))
    got = emu.chroma(case)
    B.check_scaled_chroma(got, clean, k, "emulation")
    if k not in B.CHROMA_ZERO:
        assert got[:, 38].all()
        worst, left_out = check_records(got, case, f"2^{k}")
        assert left_out <= GUARD_SHARE * len(got) and worst <= 0.25, (k, worst, left_out)


def test_window_sums_on_the_cpu(emu, cases):
    rec = cases["c_major"].ref.astype(np.float32)
    rec[40, 3], rec[41, 36], rec[42] = np.nan, np.inf, -np.inf
    for first, frames in ((0, 1), (5, 2), (30, 37), (0, len(rec)), (7, 0)):
        assert emu.sum(rec, first, frames).tobytes() == K.chroma_sum(rec, first, frames).tobytes(), (first, frames)


# ---- the host logic against the reference, field for field ----
def same_key(got, want, what):
    for k in KEY_FIELDS:
        assert got[k] == want[k] or (isinstance(want[k], float) and math.isnan(want[k]) and math.isnan(got[k])), (what, k, got[k], want[k])


def one_class(c, weight=3.0, tuning=0.0):
    """A sum holding one pitch class, its phasor at `tuning` cents."""
    S = np.zeros(K.COLS)
    S[3 * c] = weight
    S[36], S[37], S[38] = weight * math.cos(2 * math.pi * tuning / 100), weight * math.sin(2 * math.pi * tuning / 100), weight
    return S


def bare_fifth():
    """A and E alone: no third, so nothing but the profiles' own shapes separates A major from A minor."""
    S = np.zeros(K.COLS)
    S[0] = S[21] = 1.0
    S[36] = S[38] = 2.0
    return S


def test_key_from_chroma_crafted(mxlib):
    zeros = np.zeros(K.COLS)
    got = mxlib.key_from_chroma(zeros)
    same_key(got, K.key_from_sum(zeros), "zeros")
    assert got["scale_mask"] == 0 and got["clarity"] == 0.0 and got["tuning_cents"] == 0.0
    flat = np.zeros(K.COLS)
    flat[:36], flat[38] = 1.0, 36.0
    same_key(mxlib.key_from_chroma(flat), K.key_from_sum(flat), "flat")
    assert mxlib.key_from_chroma(flat)["scale_mask"] in (0, K.key_from_sum(flat)["scale_mask"])
    for c in range(12):
        S = one_class(c)
        got = mxlib.key_from_chroma(S)
        same_key(got, K.key_from_sum(S), f"class {c}")
        assert got["tonic"] == c and got["scale_mask"] >> c & 1
    fifth = bare_fifth()
    got = mxlib.key_from_chroma(fifth)
    same_key(got, K.key_from_sum(fifth), "fifth")
    # a major / minor tie: the sum of the two standardised key profiles on one tonic correlates alike with both (to the last
    # bits of the sums: the winner is then whichever the reference's own arithmetic names, and clarity is nothing)
    tie = np.zeros(K.COLS)
    zm = [(a - sum(K.MAJOR) / 12) / math.sqrt(sum((x - sum(K.MAJOR) / 12) ** 2 for x in K.MAJOR)) for a in K.MAJOR]
    zn = [(a - sum(K.MINOR) / 12) / math.sqrt(sum((x - sum(K.MINOR) / 12) ** 2 for x in K.MINOR)) for a in K.MINOR]
    for c in range(12):
        tie[3 * c] = 1.0 + 0.5 * (zm[c] + zn[c])
    tie[36] = tie[38] = tie[:36].sum()
    got, want = mxlib.key_from_chroma(tie), K.key_from_sum(tie)
    same_key(got, want, "tie")
    assert got["tonic"] == 0 and abs(got["clarity"]) < 1e-12 and got["mode"] == want["mode"]
    for t, expect in ((50.0, 50.0), (-50.0, 50.0), (49.999, 49.999), (-49.999, -49.999)):
        S = one_class(3, tuning=t)
        if abs(t) == 50.0:
            S[37] = 0.0 if t > 0 else -0.0  # atan2(+-0, -1) = +-pi: both ends of the range are +50
        got = mxlib.key_from_chroma(S)
        same_key(got, K.key_from_sum(S), f"tuning {t}")
        assert abs(got["tuning_cents"] - expect) < 1e-9 and -50.0 < got["tuning_cents"] <= 50.0
    for bad in (np.nan, np.inf, -np.inf):
        for col in (0, 17, 36, 37, 38, 39):
            S = one_class(5, tuning=12.0) + one_class(9, 1.0, tuning=12.0)
            S[col] = bad
            got = mxlib.key_from_chroma(S)
            same_key(got, K.key_from_sum(S), f"{bad} in column {col}")
            assert all(math.isfinite(got[k]) for k in KEY_FIELDS)


def test_key_from_chroma_random(mxlib):
    rng = np.random.default_rng(0x6B6579)
    for i in range(300):
        S = np.zeros(K.COLS)
        S[:36] = rng.random(36) ** rng.integers(1, 6)
        ang = rng.uniform(-math.pi, math.pi)
        S[38] = S[:36].sum()
        r = rng.random() * S[38]
        S[36], S[37] = r * math.cos(ang), r * math.sin(ang)
        if i % 7 == 0:
            S[rng.integers(0, 40)] = rng.choice([np.nan, np.inf, 0.0, -1.0])
        same_key(mxlib.key_from_chroma(S), K.key_from_sum(S), i)


def notes_array(mxlib, notes):
    """(note, frames) pairs -> NOTE_DTYPE, laid out one behind the other."""
    out = np.zeros(len(notes), dtype=mxlib.NOTE_DTYPE)
    for i, (note, frames) in enumerate(notes):
        out[i] = (1000 * i + 1, 1000 * i + 900, 4 * i, frames, note, 0.05, 0.1)
    return out


def test_key_from_notes(mxlib):
    same_key(mxlib.key_from_notes(notes_array(mxlib, [])), K.key_from_notes([]), "no notes")
    assert mxlib.key_from_notes(notes_array(mxlib, []))["scale_mask"] == 0
    one = [(51.2, 10)]
    got = mxlib.key_from_notes(notes_array(mxlib, one))
    same_key(got, K.key_from_notes(one), "one note")
    assert got["tonic"] == 3 and abs(got["tuning_cents"] - 20.0) < 1e-9
    overlapping = notes_array(mxlib, [(51.0, 20), (58.0, 20), (55.0, 10)])
    overlapping["start_sample"], overlapping["end_sample"] = [5, 5, 5], [900, 400, 2000]
    same_key(mxlib.key_from_notes(overlapping), K.key_from_notes([(51.0, 20), (58.0, 20), (55.0, 10)]), "overlapping")
    for t in (0.0, 23.45, -35.0, 49.0, -49.0, 50.0):
        mel = [(48 + k + t / 100.0, 12 + (i % 3)) for i, k in enumerate(K.C_MAJOR)]
        got = mxlib.key_from_notes(notes_array(mxlib, mel))
        same_key(got, K.key_from_notes(mel), f"C major at {t}")
        assert (got["tonic"], got["mode"], got["scale_mask"]) == (3, 0, K.scale_mask(3, 0)) and abs(got["tuning_cents"] - t) < 1e-6
        assert got["tuning_confidence"] > 0.999
    mel = [(48 + k, 12) for k in K.A_MINOR]
    got = mxlib.key_from_notes(notes_array(mxlib, mel))
    same_key(got, K.key_from_notes(mel), "A minor")
    assert (got["tonic"], got["mode"]) == (0, 1)
    rng = np.random.default_rng(5)
    for i in range(100):
        mel = [(float(rng.uniform(-30, 110)), int(rng.integers(-2, 40))) for _ in range(rng.integers(1, 30))]
        same_key(mxlib.key_from_notes(notes_array(mxlib, mel)), K.key_from_notes(mel), i)
    with pytest.raises(mxlib.MxError):
        mxlib.key_from_notes(notes_array(mxlib, [(float("nan"), 3)]))


def ref_notes(notes):
    """NOTE_DTYPE records as yin_ref's tuples."""
    return [(int(n["start_sample"]), int(n["end_sample"]), int(n["first_frame"]), int(n["frames"]), float(n["note"])) for n in notes]


def test_correction_markers_tuned(mxlib):
    rng = np.random.default_rng(11)
    notes = notes_array(mxlib, [(float(rng.uniform(30, 80)), 10) for _ in range(40)] + [(51.5, 5), (52.0, 5), (-3.5, 4)])
    for mask in (0, K.scale_mask(3, 0), K.scale_mask(0, 1), 1 << 7):
        for strength in (1.0, 0.35, 0.0):
            plain = mxlib.correction_markers(notes, strength, mask)
            assert mxlib.correction_markers_tuned(notes, strength, mask, 0.0).tobytes() == plain.tobytes()  # tuning 0: the old call's bytes
            for t in (23.45, -35.0, 50.0, -50.0, 0.125):
                got = mxlib.correction_markers_tuned(notes, strength, mask, t)
                want = K.markers_tuned(ref_notes(notes), strength, mask, t)
                assert [tuple(m) for m in got.tolist()] == want, (mask, strength, t)
                # notes shifted by t/100 on the grid shifted by t: the unshifted call's bends
                shifted = notes.copy()
                shifted["note"] = notes["note"] + t / 100.0
                bends = mxlib.correction_markers_tuned(shifted, strength, mask, t)["pitchBend"]
                np.testing.assert_allclose(bends, plain["pitchBend"], rtol=0, atol=1e-12)
    assert len(mxlib.correction_markers_tuned(notes[:0], 1.0, 0, 10.0)) == 0


def test_refusals(mxlib):
    notes = notes_array(mxlib, [(50.0, 10), (52.0, 10)])

    def refused(fn, *args):
        with pytest.raises(mxlib.MxError) as e:
            fn(*args)
        assert e.value.code == -1, args

    # what mx_correction_markers refuses ...
    for args in ((notes, 1.5, 0), (notes, -0.1, 0), (notes, float("nan"), 0), (notes, 1.0, -1), (notes, 1.0, 0x1000)):
        refused(mxlib.correction_markers, *args)
        refused(mxlib.correction_markers_tuned, *args, 0.0)
    for spoil in ("order", "overlap", "nan", "empty"):
        bad = notes.copy()
        if spoil == "order":
            bad = bad[::-1].copy()
        elif spoil == "overlap":
            bad["start_sample"][1] = bad["end_sample"][0]
        elif spoil == "nan":
            bad["note"][1] = np.inf
        else:
            bad["end_sample"][0] = bad["start_sample"][0]
        refused(mxlib.correction_markers, bad, 1.0, 0)
        refused(mxlib.correction_markers_tuned, bad, 1.0, 0, 0.0)
    # ... and a tuning outside the half semitone either side
    for t in (50.001, -50.001, float("nan"), float("inf")):
        refused(mxlib.correction_markers_tuned, notes, 1.0, 0, t)
    L = mxlib._capi.lib()
    key = mxlib._capi.Key()
    assert L.mx_key_from_chroma(None, C.byref(key)) == -1 and L.mx_key_from_chroma(np.zeros(40).ctypes.data, None) == -1
    assert L.mx_key_from_notes(None, 1, C.byref(key)) == -1 and L.mx_key_from_notes(None, -1, C.byref(key)) == -1
    assert L.mx_key_from_notes(None, 0, None) == -1
    with pytest.raises(ValueError):
        mxlib.key_from_chroma(np.zeros(39))
    assert mxlib.chroma_params_default() == K.CHROMA_DEFAULTS


def test_the_stand_alone_program_under_the_sanitizers(tmp_path):
    """The emulation and the library's host logic with a main of their own over the smallest shapes, the longest peak list and
    the edges of every list, under AddressSanitizer and UBSan."""
    out = emu_build.run_sanitized(tmp_path, "chroma_emu_san", ["chroma_emu.cpp", "key_logic.cpp", "f0_notes.cpp"], "CHROMA_EMU_MAIN",
                                  opt=("-O1",))  # (the transform's templates at -O2 -g under ASan compile for a minute)
    assert "chroma_emu ok" in out, out


def test_chroma_kernels_do_not_spill():
    """Both kernels scratch-free inside 256 VGPRs; the frame kernel's LDS is the FFT image, the pass-2 twiddles, the padded
    magnitude image and four words."""
    names, scratch, vgprs, lds = emu_build.resource_usage("chroma_kernels.hip")
    lds = dict(zip(names, lds))
    assert len(names) == 2
    assert scratch == [0, 0] and max(vgprs) <= 256, (scratch, vgprs)
    frames = next(n for n in names if "chroma_frames" in n)
    assert lds[frames] == 16384 + 8 * 240 + 4 * (2048 + 128) + 16 and lds[next(n for n in names if "chroma_sum" in n)] == 0


# ---- the reference, and the library's host logic on the reference's records, against the truth ----
def test_the_takes_key_scale_and_tuning(mxlib, cases):
    worst, clarities = 0.0, {}
    for name, (w, tonic, mode, tuning) in K.takes().items():
        rec = cases[name].ref.astype(np.float32)
        want = K.key_from_sum(K.chroma_sum(rec, 0, len(rec)))
        got = mxlib.key_from_chroma(K.chroma_sum(rec, 0, len(rec)))
        same_key(got, want, name)
        print(f"{name}: tonic {got['tonic']} mode {got['mode']} tuning {got['tuning_cents']:+.3f} (truth {tuning:+.3f}) "
              f"correlation {got['correlation']:.3f} clarity {got['clarity']:.3f} confidence {got['tuning_confidence']:.3f}")
        assert (got["tonic"], got["mode"], got["scale_mask"]) == (tonic, mode, K.scale_mask(tonic, mode)), name
        assert abs(got["tuning_cents"] - tuning) <= TUNING_BOUND, name
        worst = max(worst, abs(got["tuning_cents"] - tuning))
        clarities[name] = got["clarity"]
    print(f"worst tuning error of the reference: {worst:.3f} cents (bound {TUNING_BOUND})")
    assert 3.0 * worst <= TUNING_BOUND
    assert K.scale_mask(3, 0) == K.scale_mask(0, 1) == 0b010110101101  # C major = A minor: A B C D E F G
    # white noise and silence: no key to speak of — clarity under every take's by 0.05 on the reference, mask 0 for silence
    noise = K.key_detect(K.noise(), SR)[0]
    silence = K.key_detect(np.zeros(SR, dtype=np.float32), SR)[0]
    print(f"noise: clarity {noise['clarity']:.3f} confidence {noise['tuning_confidence']:.4f}; takes' clarity {min(clarities.values()):.3f} and up")
    assert noise["clarity"] < min(clarities.values()) - 0.05 and noise["tuning_confidence"] < 0.05
    assert silence["scale_mask"] == 0 and silence["clarity"] == 0.0 and silence["tuning_cents"] == 0.0
    same_key(mxlib.key_from_chroma(np.zeros(K.COLS)), silence, "silence")


def test_windows_of_a_take(cases):
    assert K.windows(10, 4, 3) == [(0, 4), (3, 4), (6, 4), (9, 1)] and K.windows(10, 0, 1) == [] and K.windows(0, 4, 1) == []
    rec = cases["c_major"].ref.astype(np.float32)
    take, wins = K.key_detect(None, SR, window_frames=48, window_hop=24, rec=rec)
    assert len(wins) == 6 and all(abs(k["tuning_cents"] - take["tuning_cents"]) < 2.0 for _, _, k in wins)


# ---- the whole correction chain on the references ----
CHAIN_DETUNE = (-30.0, 20.0, -10.0, 30.0, 10.0, -20.0, 0.0)  # cents off the 446 Hz grid, note after note
# How far a re-detected note may sit from the 446 Hz C-major grid after the tuned chain.  On the references (below) the worst is
# 4.9 cents — the one note the tracker cuts from two tones of different detuning ("3 3"), which one bend cannot put right — and
# 2.1 cents for every other note: the estimate's own offset (21.35 against 23.45 cents: the pattern's mean over 24 notes is
# -0.8 cents and the partials' offset adds).  The plain chain (mask 0, A = 440 Hz) leaves every note 23.4 cents off.
CHAIN_BOUND, CHAIN_TYPICAL, CHAIN_PLAIN_MISS = 8.0, 3.0, 15.0


def off_grid(notes, tuning):
    """cents of each note (its `note` value) from the nearest semitone of the grid `tuning` cents above A = 440 Hz."""
    v = np.array([float(n) for n in notes]) - tuning / 100.0
    return (v - np.rint(v)) * 100.0


def check_chain(tuned_notes, plain_notes, what):
    truth = 1200.0 * math.log2(446.0 / 440.0)
    tuned, plain = off_grid(tuned_notes, truth), off_grid(plain_notes, truth)
    print(f"{what}: tuned chain worst {np.abs(tuned).max():.2f} median {np.median(np.abs(tuned)):.2f} cents off the 446 Hz grid; "
          f"plain chain median {np.median(np.abs(plain)):.2f}")
    assert len(tuned_notes) >= 20 and np.abs(tuned).max() <= CHAIN_BOUND and np.median(np.abs(tuned)) <= CHAIN_TYPICAL, what
    classes = np.rint(np.array([float(n) for n in tuned_notes]) - truth / 100.0).astype(int) % 12
    assert all(K.scale_mask(3, 0) >> c & 1 for c in classes), what
    assert np.median(np.abs(plain)) >= CHAIN_PLAIN_MISS, what


def test_the_reference_chain_lands_on_the_detected_grid():
    import psola_ref as P

    hop = 256
    f0 = np.dtype([("tau", "<i4"), ("period", "<f4"), ("aperiodicity", "<f4"), ("rms", "<f4")])

    def notes_of(w):
        tr = np.array([tuple(r) for r in Y.track(w, SR, hop)[0]], dtype=f0)
        return tr, Y.detect_notes(tr, SR, hop)

    w = K.melody(K.C_MAJOR, 446.0, detune=CHAIN_DETUNE)
    tr, notes = notes_of(w)
    key = K.key_detect(w, SR)[0]
    assert (key["tonic"], key["mode"]) == (3, 0) and abs(key["tuning_cents"] - 23.45) < 3.0
    out = []
    for markers in (K.markers_tuned(notes, 1.0, key["scale_mask"], key["tuning_cents"]), Y.correction_markers(notes, 1.0, 0)):
        grains, length = P.plan(len(w), SR, hop, tr, markers)
        out.append([n[4] for n in notes_of(np.asarray(P.render(w, grains, length), dtype=np.float32))[1]])
    check_chain(out[0], out[1], "references")
