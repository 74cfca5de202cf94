"""xd-tts hot path on MI355X: Python mirror of the reference's Rust surface over the C ABI.

The product is ``libxdtts_hip.so`` (HIP kernels + ``extern "C"`` entry points, declared in
``include/xdtts.h``).  This module is the thin host-side binding used by tests and bench.py; it
mirrors the reference's operator interface for the hot path:

* ``Tacotron2.load(path)`` / ``Tacotron2.infer(ids)``   -- src/tacotron2/mod.rs:242,398
* ``create_mel_filter_bank(...)``                       -- griffin_lim::mel, src/tacotron2/mod.rs:453
* ``GriffinLim(mel_basis, noverlap, power, iter, momentum)`` / ``.infer(mel)``
                                                        -- src/tacotron2/mod.rs:456, src/lib.rs:141
* ``create_griffin_lim()``                              -- src/tacotron2/mod.rs:441-458

There is no CPU fallback: if the shared library is missing, importing fails; if no HIP device is
visible every call raises ``XdttsError`` (status XDTTS_ERR_NO_DEVICE).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("XDTTS_LIB") or os.path.join(_HERE, "libxdtts_hip.so")  # XDTTS_LIB: developer builds (profiling)

N_MEL = 80
EMB = 512
ATT_DIM = 128

STATUS = {0: "OK", 1: "BAD_ARG", 2: "IO", 3: "HIP", 4: "OOM", 5: "TOO_LONG", 6: "NO_DEVICE"}
XDTTS_ERR_BAD_ARG, XDTTS_ERR_IO, XDTTS_ERR_HIP, XDTTS_ERR_OOM, XDTTS_ERR_TOO_LONG, XDTTS_ERR_NO_DEVICE = 1, 2, 3, 4, 5, 6


class XdttsError(RuntimeError):
    """Non-zero xdtts_status; the Rust shim maps this to anyhow::Error (mod.rs:249,254,259)."""

    def __init__(self, status, message):
        super().__init__("xdtts status %d (%s): %s" % (status, STATUS.get(status, "?"), message))
        self.status = status


class GriffinLimOpts(C.Structure):
    """xdtts_griffinlim_opts: the conventions of GriffinLim::infer's mel->linear step as switches."""

    _fields_ = [("nnls_iters", C.c_int32), ("power_mode", C.c_int32), ("mel_decompress", C.c_int32), ("output_normalise", C.c_int32), ("batch_shape", C.c_int32), ("rms_target", C.c_float)]


class Prosody(C.Structure):
    """xdtts_prosody: speaking rate and pitch, applied to the linear magnitude between mel -> linear and the Griffin-Lim loop.
    rate in [0.25, 4] (> 1: faster), pitch in [0.5, 2] (> 1: higher), lifter in [1, 255] cepstral bins of envelope, log_floor > 0.
    Prosody() holds the library's defaults (1, 1, 30, 1e-5), i.e. the identity; keywords override fields."""

    _fields_ = [("rate", C.c_float), ("pitch", C.c_float), ("lifter", C.c_int32), ("log_floor", C.c_float)]

    def __init__(self, **kw):
        super().__init__()
        lib.xdtts_prosody_default(C.byref(self))
        for k, v in kw.items():
            setattr(self, k, v)


class Timbre(C.Structure):
    """xdtts_timbre: the voice of a vocoder handle, applied to the magnitude behind the prosody stage and in front of the initial
    phase.  vtl in [0.5, 2] (> 1: a longer vocal tract, formants move down, F0 stays), breath in [0, 1] (1: a whisper), seed of
    the breath noise, lifter in [1, 255], log_floor > 0.  Timbre() holds the library's defaults (1, 0, 1, 30, 1e-5), i.e. the
    identity; keywords override fields."""

    _fields_ = [("vtl", C.c_float), ("breath", C.c_float), ("seed", C.c_uint32), ("lifter", C.c_int32), ("log_floor", C.c_float)]

    def __init__(self, **kw):
        super().__init__()
        lib.xdtts_timbre_default(C.byref(self))
        for k, v in kw.items():
            setattr(self, k, v)

    def astuple(self):
        return (self.vtl, self.breath, self.seed, self.lifter, self.log_floor)


class DurationsOpts(C.Structure):
    """xdtts_durations_opts: the durations setting of a mel-generator handle.  on in {0, 1}; an id under min_frames counts as
    skipped, one over max_frames as stuck (0 <= min_frames <= max_frames <= 65535).  DurationsOpts() holds the library's defaults
    (off, 0.5, 40); keywords override fields."""

    _fields_ = [("on", C.c_int32), ("min_frames", C.c_float), ("max_frames", C.c_float)]

    def __init__(self, **kw):
        super().__init__()
        lib.xdtts_durations_default(C.byref(self))
        for k, v in kw.items():
            setattr(self, k, v)


class AlignmentStats(C.Structure):
    """xdtts_alignment_stats: per utterance, from the Q16 durations."""

    _fields_ = [("sum_q16", C.c_uint64), ("n_frames", C.c_uint64), ("n_ids", C.c_uint32), ("min_q16", C.c_uint32), ("min_index", C.c_uint32),
                ("max_q16", C.c_uint32), ("max_index", C.c_uint32), ("n_below", C.c_uint32), ("n_above", C.c_uint32), ("last_q16", C.c_uint32)]

    def astuple(self):
        return tuple(getattr(self, f[0]) for f in self._fields_)


class Denoise(C.Structure):
    """xdtts_denoise: the clean-up stage of a vocoder handle, the first stage on the magnitude behind mel -> linear.  strength in
    [0, 16] (over-subtraction factor, 0 = none), quantile in [0, 1] (which order statistic over an utterance's frames is the
    noise), floor_db in [-80, 0] (the most a cell is attenuated), tone = up to 8 (hz, dB) points, hz strictly ascending in
    (0, 11025], dB in [-40, 20].  Denoise() holds the library's defaults (0, 0.5, -20, no tone), i.e. the identity; keywords
    override fields: Denoise(strength=2, tone=[(300, -6), (3400, 0)])."""

    _fields_ = [("strength", C.c_float), ("quantile", C.c_float), ("floor_db", C.c_float), ("n_tone", C.c_int32),
                ("tone_hz", C.c_float * 8), ("tone_db", C.c_float * 8)]

    def __init__(self, tone=None, **kw):
        super().__init__()
        lib.xdtts_denoise_default(C.byref(self))
        for k, v in kw.items():
            setattr(self, k, v)
        if tone is not None:
            pts = [(float(h), float(d)) for h, d in tone]
            if len(pts) > 8:
                raise ValueError("a tone curve has at most 8 points, got %d" % len(pts))
            self.n_tone = len(pts)
            for i, (h, d) in enumerate(pts):
                self.tone_hz[i], self.tone_db[i] = h, d

    def astuple(self):
        return (self.strength, self.quantile, self.floor_db, self.n_tone, tuple(self.tone_hz), tuple(self.tone_db))


class DenoiseStats(C.Structure):
    """xdtts_denoise_stats of one utterance: cells = 513 F, floored = the cells at the spectral floor, rank = r of the selection
    (0 where none ran), profiled = 1 where the subtraction ran against a caller's profile."""

    _fields_ = [("cells", C.c_uint32), ("floored", C.c_uint32), ("rank", C.c_uint32), ("profiled", C.c_uint32)]

    def astuple(self):
        return (self.cells, self.floored, self.rank, self.profiled)


class ProsodyPoint(C.Structure):
    """xdtts_prosody_point: (pos, rate, pitch, gain), pos a fraction of the utterance's duration in [0, 1]."""

    _fields_ = [("pos", C.c_float), ("rate", C.c_float), ("pitch", C.c_float), ("gain", C.c_float)]


class ProsodyContour(C.Structure):
    """xdtts_prosody_contour: rate, pitch and gain that vary inside one utterance.  ProsodyContour([(pos, rate, pitch, gain), ...])
    -- pos in [0, 1] and non-decreasing (two points at one pos make a step), rate in [0.25, 4], pitch in [0.5, 2], gain in [0, 8];
    values are interpolated linearly between the points and held before the first and after the last.  lifter and log_floor as
    in Prosody.  The identity (every point 1, 1, 1) launches nothing."""

    _fields_ = [("points", C.POINTER(ProsodyPoint)), ("n_points", C.c_int32), ("lifter", C.c_int32), ("log_floor", C.c_float)]

    def __init__(self, points=(), lifter=None, log_floor=None):
        super().__init__()
        lib.xdtts_prosody_contour_default(C.byref(self))
        pts = [tuple(float(x) for x in p) for p in points]
        if any(len(p) != 4 for p in pts):
            raise ValueError("a contour point is (pos, rate, pitch, gain)")
        self._pts = (ProsodyPoint * max(len(pts), 1))(*pts)  # kept alive with the struct
        self.points = C.cast(self._pts, C.POINTER(ProsodyPoint)) if pts else None
        self.n_points = len(pts)
        if lifter is not None:
            self.lifter = lifter
        if log_floor is not None:
            self.log_floor = log_floor


class F0Opts(C.Structure):
    """xdtts_f0_opts: the pitch tracker's search range in Hz (50 <= fmin < fmax <= 1000), the voicing threshold on the cepstral
    peak (>= 0), octave_bias in (0, 1] (1 = the plain argmax; lower prefers the first peak over a rahmonic) and log_floor > 0.
    F0Opts() holds the library's defaults (60, 400, 0.2, 0.9, 1e-5); keywords override fields."""

    _fields_ = [("fmin", C.c_float), ("fmax", C.c_float), ("threshold", C.c_float), ("octave_bias", C.c_float), ("log_floor", C.c_float)]

    def __init__(self, **kw):
        super().__init__()
        lib.xdtts_f0_opts_default(C.byref(self))
        for k, v in kw.items():
            setattr(self, k, v)


PITCH_NONE, PITCH_HZ, PITCH_FACTOR = 0, 1, 2


class PitchTarget(C.Structure):
    """xdtts_pitch_target: mode 0 none, 1 `value` an absolute median pitch in Hz (50 .. 1000), 2 `value` a factor (0.5 .. 2);
    range in [0, 4] scales every frame's excursion from the median in log-frequency (1 leaves it, 0 flattens, 2 doubles).
    PitchTarget() is the identity {0, 1, 1}; PitchTarget(hz=180), PitchTarget(factor=1.1, range=0.5)."""

    _fields_ = [("mode", C.c_int32), ("value", C.c_float), ("range", C.c_float)]

    def __init__(self, hz=None, factor=None, range=None, mode=None, value=None):
        super().__init__()
        lib.xdtts_pitch_target_default(C.byref(self))
        if hz is not None and factor is not None:
            raise ValueError("pass hz= or factor=, not both")
        if hz is not None:
            self.mode, self.value = PITCH_HZ, hz
        if factor is not None:
            self.mode, self.value = PITCH_FACTOR, factor
        if mode is not None:
            self.mode = mode
        if value is not None:
            self.value = value
        if range is not None:
            self.range = range


class F0Stats(C.Structure):
    """xdtts_f0_stats: what the tracker found in one utterance, and what a target did with it."""

    _fields_ = [("n_frames", C.c_int32), ("n_voiced", C.c_int32), ("n_clamped", C.c_int32), ("median_hz", C.c_float), ("min_hz", C.c_float),
                ("max_hz", C.c_float), ("base_ratio", C.c_float)]

    def astuple(self):
        return (self.n_frames, self.n_voiced, self.n_clamped, self.median_hz, self.min_hz, self.max_hz, self.base_ratio)

    def bits(self):
        """The struct's bytes: what `bit for bit` compares (a float's NaN or -0 included)."""
        return bytes(self)


class Loudness(C.Structure):
    """xdtts_loudness: the BS.1770 measurement of one utterance and the gain that was applied.  .lufs is the integrated
    loudness (-inf where no block passed the gates)."""

    _fields_ = [("mean_square", C.c_double), ("true_peak", C.c_double), ("sample_peak", C.c_double), ("gain", C.c_double),
                ("blocks", C.c_int32), ("gated_blocks", C.c_int32)]

    @property
    def lufs(self):
        return float(lib.xdtts_loudness_lufs(C.byref(self)))

    def astuple(self):
        return (self.mean_square, self.true_peak, self.sample_peak, self.gain, self.blocks, self.gated_blocks)


class LimiterStats(C.Structure):
    """xdtts_limiter_stats: what the look-ahead limiter did to one utterance."""

    _fields_ = [("min_gain", C.c_float), ("half_width", C.c_int32), ("engaged", C.c_int32), ("limited", C.c_int64)]

    def astuple(self):
        return (self.min_gain, self.half_width, self.engaged, self.limited)


class Compressor(C.Structure):
    """xdtts_compressor: the dynamic range compressor in front of the level stage.  threshold_db in [-60, 0] (dB under the
    utterance's own sample peak), ratio in [1, 20], knee_db in [0, 24], attack_ms in [0.1, 100], release_ms in [1, 2000],
    makeup_db in [0, 24].  Compressor() holds the library's defaults (0, 1, 0, 5, 100, 0), i.e. the identity; keywords override
    fields; compressor_preset(1) is "drc"."""

    _fields_ = [("threshold_db", C.c_float), ("ratio", C.c_float), ("knee_db", C.c_float), ("attack_ms", C.c_float), ("release_ms", C.c_float),
                ("makeup_db", C.c_float)]

    def __init__(self, **kw):
        super().__init__()
        lib.xdtts_compressor_default(C.byref(self))
        for k, v in kw.items():
            setattr(self, k, v)

    def astuple(self):
        return (self.threshold_db, self.ratio, self.knee_db, self.attack_ms, self.release_ms, self.makeup_db)


class CompressorStats(C.Structure):
    """xdtts_compressor_stats: what the compressor did to one utterance."""

    _fields_ = [("peak", C.c_float), ("max_over", C.c_int32), ("engaged", C.c_int32), ("compressed", C.c_int64)]

    def astuple(self):
        return (self.peak, self.max_over, self.engaged, self.compressed)


class Silence(C.Structure):
    """xdtts_silence: the silence stage, the last of the delivery chain.  threshold_db in [-96, -6] (dB under the utterance's own
    sample peak), min_sound_ms in [0, 500], lead_ms and trail_ms in [0, 10000], max_pause_ms 0 (pauses untouched) or in
    [20, 60000], fade_ms in [0, 2.5].  Silence() holds the library's defaults (-40, 20, 50, 100, 0, 2); keywords override fields."""

    _fields_ = [("threshold_db", C.c_float), ("min_sound_ms", C.c_float), ("lead_ms", C.c_float), ("trail_ms", C.c_float),
                ("max_pause_ms", C.c_float), ("fade_ms", C.c_float)]

    def __init__(self, **kw):
        super().__init__()
        lib.xdtts_silence_default(C.byref(self))
        for k, v in kw.items():
            setattr(self, k, v)

    def astuple(self):
        return (self.threshold_db, self.min_sound_ms, self.lead_ms, self.trail_ms, self.max_pause_ms, self.fade_ms)


class SilenceStats(C.Structure):
    """xdtts_silence_stats: what the silence stage did to one utterance."""

    _fields_ = [("n_in", C.c_uint32), ("n_out", C.c_uint32), ("lead_cut", C.c_uint32), ("trail_cut", C.c_uint32), ("pause_cut", C.c_uint32),
                ("n_cuts", C.c_uint32), ("peak", C.c_float), ("any_sound", C.c_uint32)]

    def astuple(self):
        return (self.n_in, self.n_out, self.lead_cut, self.trail_cut, self.pause_cut, self.n_cuts, self.peak, self.any_sound)


STREAM_F32, STREAM_PCM16, STREAM_ULAW, STREAM_ALAW = 0, 1, 2, 3
_STREAM_DTYPE = {STREAM_F32: np.float32, STREAM_PCM16: np.dtype("<i2"), STREAM_ULAW: np.uint8, STREAM_ALAW: np.uint8}


class StreamOpts(C.Structure):
    """xdtts_stream_opts: how a joined sequence leaves the device.  format 0 fp32, 1 PCM16, 2 G.711 mu-law, 3 A-law; dither 1 =
    TPDF (PCM16 only) seeded by dither_seed and the absolute stream position; level 1 = programme (ONE BS.1770 gain for the
    whole stream, needs set_loudness); fade = samples per utterance edge at the delivered rate (0 .. 4800)."""

    _fields_ = [("format", C.c_int32), ("dither", C.c_int32), ("dither_seed", C.c_uint32), ("level", C.c_int32), ("fade", C.c_int32)]

    def __init__(self, format=None, dither=None, dither_seed=None, level=None, fade=None):
        super().__init__()
        lib.xdtts_stream_opts_default(C.byref(self))
        for k, v in (("format", format), ("dither", dither), ("dither_seed", dither_seed), ("level", level), ("fade", fade)):
            if v is not None:
                setattr(self, k, int(v))


class InferOpts(C.Structure):
    _fields_ = [
        ("gate_threshold", C.c_float),
        ("max_steps", C.c_int32),
        ("fixed_steps", C.c_int32),
        ("dropout_mode", C.c_int32),
        ("dropout_seed", C.c_uint32),
        ("max_chunk", C.c_int32),
        ("item_base", C.c_uint32),
        ("fixed_frames_per_id", C.c_float),
        ("dropout_masks", C.c_void_p),      # dropout_mode 2: keep bytes [chunk][steps][2][256]
        ("dropout_mask_steps", C.c_int32),
    ]


# name -> (restype, argtypes).  Every symbol include/xdtts.h declares is listed here; the CPU-only
# tests check that the library exports all of them.
_VP, _I32, _U32, _SZ, _F = C.c_void_p, C.c_int32, C.c_uint32, C.c_size_t, C.c_float
_PF = C.POINTER(C.c_float)
SYMBOLS = {
    "xdtts_infer_opts_default": (None, [C.POINTER(InferOpts)]),
    "xdtts_tacotron2_load": (_I32, [C.c_char_p, _I32, C.POINTER(_VP)]),
    "xdtts_model_dir_read": (_I32, [C.c_char_p, _VP, _SZ]),
    "xdtts_model_dir_describe": (_I32, [C.c_char_p, C.c_char_p, _SZ, C.POINTER(_SZ)]),
    "xdtts_tacotron2_load_synthetic": (_I32, [_U32, _F, _I32, C.POINTER(_VP)]),
    "xdtts_tacotron2_load_blob": (_I32, [_VP, _SZ, _I32, C.POINTER(_VP)]),
    "xdtts_tacotron2_save": (_I32, [_VP, C.c_char_p]),
    "xdtts_tensor_count": (_I32, []),
    "xdtts_tensor_name": (C.c_char_p, [_I32]),
    "xdtts_tensor_ndim": (_I32, [_I32]),
    "xdtts_tensor_dim": (_I32, [_I32, _I32]),
    "xdtts_tensor_offset": (_SZ, [_I32]),
    "xdtts_tensor_total": (_SZ, []),
    "xdtts_tacotron2_get_tensor": (_I32, [_VP, _I32, _VP]),
    "xdtts_tacotron2_infer_ids": (_I32, [_VP, _VP, _SZ, _VP, _SZ, C.POINTER(InferOpts), C.POINTER(_PF), C.POINTER(_SZ)]),
    "xdtts_tacotron2_infer_batch": (_I32, [_VP, _VP, _VP, _I32, _I32, C.POINTER(InferOpts), _VP, C.POINTER(_PF), C.POINTER(_SZ)]),
    "xdtts_tacotron2_encoder": (_I32, [_VP, _VP, _I32, _VP, _VP]),
    "xdtts_tacotron2_encoder_batch": (_I32, [_VP, _I32, _VP, _I32, _I32, _VP, _VP]),
    "xdtts_tacotron2_decoder": (_I32, [_VP, _VP, _VP, _I32, _I32, C.POINTER(InferOpts), _VP, _VP, C.POINTER(_SZ)]),
    "xdtts_tacotron2_decoder_step": (_I32, [_VP, _VP, _VP, _I32, _I32, C.POINTER(InferOpts), _U32] + [_VP] * 10),
    "xdtts_tacotron2_decoder_steps": (_I32, [_VP, _I32, _I32, _VP, _VP, _I32, _VP, C.POINTER(InferOpts), _U32, _I32] + [_VP] * 10),
    "xdtts_tacotron2_engine_state": (_I32, [_VP, C.POINTER(_I32), C.POINTER(_I32), C.POINTER(_I32)]),
    "xdtts_tacotron2_small_batch_engine_state": (_I32, [_VP, C.POINTER(_I32)]),
    "xdtts_tacotron2_engine_reset": (_I32, [_VP]),
    "xdtts_tacotron2_postnet": (_I32, [_VP, _VP, _I32, _VP]),
    "xdtts_tacotron2_postnet_batch": (_I32, [_VP, _VP, _SZ, _VP, _I32, _I32, _VP]),
    "xdtts_tacotron2_last_timings": (_I32, [_VP, C.POINTER(C.c_float * 4), C.POINTER(_I32)]),
    "xdtts_durations_default": (None, [_VP]),
    "xdtts_tacotron2_set_durations": (_I32, [_VP, _VP]),
    "xdtts_tacotron2_get_durations": (_I32, [_VP, _VP]),
    "xdtts_tacotron2_last_durations_count": (_I32, [_VP, C.POINTER(_SZ)]),
    "xdtts_tacotron2_last_durations": (_I32, [_VP, _SZ, _VP, _VP, _VP, _SZ, C.POINTER(_SZ)]),
    "xdtts_tacotron2_last_alignment": (_I32, [_VP, _SZ, _VP]),
    "xdtts_tacotron2_durations_gather": (_I32, [_VP, _VP, _VP, _I32, _I32, _VP, _VP, _VP, _I32, _VP, _VP, _VP, _VP, _VP, _SZ, _VP, _SZ, C.POINTER(_SZ), C.POINTER(_SZ)]),
    "xdtts_durations_reference": (_I32, [_VP, _VP, _I32, _I32, _VP, _VP, _VP, _I32, _VP, _VP, _VP, _VP, _VP, _SZ, _VP, _SZ, C.POINTER(_SZ), C.POINTER(_SZ)]),
    "xdtts_durations_position": (C.c_double, [_VP, _VP, _SZ, _SZ, C.c_double]),
    "xdtts_durations_samples": (C.c_int64, [C.c_uint64, _I32, C.c_int64]),
    "xdtts_tacotron2_free": (None, [_VP]),
    "xdtts_tacotron2_sync": (_I32, [_VP]),
    "xdtts_mel_filter_bank": (_I32, [_F, _SZ, _SZ, _F, _F, _VP]),
    "xdtts_griffinlim_new": (_I32, [_VP, _SZ, _SZ, _SZ, _F, _SZ, _F, _I32, C.POINTER(_VP)]),
    "xdtts_griffinlim_opts_default": (None, [_VP]),
    "xdtts_griffinlim_set_opts": (_I32, [_VP, _VP]),
    "xdtts_griffinlim_get_opts": (_I32, [_VP, _VP]),
    "xdtts_griffinlim_set_seed": (_I32, [_VP, _U32]),
    "xdtts_griffinlim_infer": (_I32, [_VP, _VP, _SZ, _SZ, C.POINTER(_PF), C.POINTER(_SZ)]),
    "xdtts_griffinlim_infer_batch": (_I32, [_VP, _VP, _SZ, _VP, _I32, _VP, _VP]),
    "xdtts_griffinlim_batch_plan": (_I32, [_VP, _VP, _I32] + [_VP] * 6),
    "xdtts_griffinlim_infer_linear": (_I32, [_VP, _VP, _VP, _SZ, _SZ, C.POINTER(_PF), C.POINTER(_SZ)]),
    "xdtts_griffinlim_mel_to_linear": (_I32, [_VP, _VP, _SZ, _SZ, _VP]),
    "xdtts_griffinlim_step": (_I32, [_VP, _VP, _VP, _VP, _SZ, _SZ]),
    "xdtts_griffinlim_last_timings": (_I32, [_VP, C.POINTER(C.c_float * 3)]),
    "xdtts_griffinlim_analysis_frames": (_SZ, [_VP, _SZ]),
    "xdtts_griffinlim_analyze": (_I32, [_VP, _VP, _SZ, _F, _VP, _VP, C.POINTER(_SZ)]),
    "xdtts_griffinlim_analyze_batch": (_I32, [_VP, _VP, _VP, _I32, _F, _VP, _VP, _VP]),
    "xdtts_griffinlim_spectral_convergence": (_I32, [_VP, _VP, _SZ, _VP, _SZ, _I32, C.POINTER(C.c_float * 2)]),
    "xdtts_griffinlim_analysis_timings": (_I32, [_VP, C.POINTER(C.c_float * 3)]),
    "xdtts_prosody_default": (None, [C.POINTER(Prosody)]),
    "xdtts_prosody_frames": (_SZ, [_SZ, _F]),
    "xdtts_griffinlim_prosody_linear": (_I32, [_VP, _VP, _SZ, C.POINTER(Prosody), _VP, C.POINTER(_SZ)]),
    "xdtts_griffinlim_infer_prosody": (_I32, [_VP, _VP, _SZ, _SZ, C.POINTER(Prosody), C.POINTER(_PF), C.POINTER(_SZ)]),
    "xdtts_griffinlim_infer_batch_prosody": (_I32, [_VP, _VP, _SZ, _VP, _I32, _VP, _VP, _VP]),
    "xdtts_griffinlim_prosody_linear_batch": (_I32, [_VP, _VP, _VP, _I32, _VP, _VP, _VP]),
    "xdtts_prosody_contour_default": (None, [C.POINTER(ProsodyContour)]),
    "xdtts_prosody_contour_frames": (_SZ, [C.POINTER(ProsodyContour), _SZ]),
    "xdtts_prosody_contour_table": (_I32, [C.POINTER(ProsodyContour), _SZ, _VP, _VP, _VP]),
    "xdtts_griffinlim_contour_linear": (_I32, [_VP, _VP, _SZ, C.POINTER(ProsodyContour), _VP, C.POINTER(_SZ)]),
    "xdtts_griffinlim_contour_linear_batch": (_I32, [_VP, _VP, _VP, _I32, _VP, _VP, _VP]),
    "xdtts_griffinlim_infer_contour": (_I32, [_VP, _VP, _SZ, _SZ, C.POINTER(ProsodyContour), C.POINTER(_PF), C.POINTER(_SZ)]),
    "xdtts_griffinlim_infer_batch_contour": (_I32, [_VP, _VP, _SZ, _VP, _I32, _VP, _VP, _VP]),
    "xdtts_f0_opts_default": (None, [C.POINTER(F0Opts)]),
    "xdtts_pitch_target_default": (None, [C.POINTER(PitchTarget)]),
    "xdtts_f0_plan": (_I32, [C.POINTER(F0Opts), C.POINTER(_I32), C.POINTER(_I32)]),
    "xdtts_f0_track_reference": (_I32, [_VP, _VP, _SZ, C.POINTER(F0Opts), C.POINTER(PitchTarget), _VP, _VP, C.POINTER(F0Stats)]),
    "xdtts_griffinlim_f0_linear": (_I32, [_VP, _VP, _SZ, C.POINTER(F0Opts), _VP, _VP, _VP, C.POINTER(F0Stats)]),
    "xdtts_griffinlim_f0_linear_batch": (_I32, [_VP, _VP, _VP, _I32, C.POINTER(F0Opts), _VP, _VP, _VP, _VP]),
    "xdtts_griffinlim_f0": (_I32, [_VP, _VP, _SZ, _SZ, C.POINTER(F0Opts), _VP, _VP, _VP, C.POINTER(F0Stats)]),
    "xdtts_griffinlim_f0_audio": (_I32, [_VP, _VP, _SZ, C.POINTER(F0Opts), _VP, _VP, _VP, C.POINTER(F0Stats)]),
    "xdtts_griffinlim_pitch_target_linear": (_I32, [_VP, _VP, _SZ, C.POINTER(F0Opts), C.POINTER(PitchTarget), C.POINTER(ProsodyContour), _VP, _VP, C.POINTER(F0Stats)]),
    "xdtts_griffinlim_pitch_target_linear_batch": (_I32, [_VP, _VP, _VP, _I32, C.POINTER(F0Opts), _VP, _VP, _VP, _VP, _VP]),
    "xdtts_griffinlim_infer_pitch_target": (_I32, [_VP, _VP, _SZ, _SZ, C.POINTER(F0Opts), C.POINTER(PitchTarget), C.POINTER(ProsodyContour), C.POINTER(_PF), C.POINTER(_SZ)]),
    "xdtts_griffinlim_infer_batch_pitch_target": (_I32, [_VP, _VP, _SZ, _VP, _I32, C.POINTER(F0Opts), _VP, _VP, _VP, _VP]),
    "xdtts_griffinlim_last_f0": (_I32, [_VP, _VP, _SZ, C.POINTER(_SZ)]),
    "xdtts_griffinlim_set_phase_init": (_I32, [_VP, _I32]),
    "xdtts_griffinlim_get_phase_init": (_I32, [_VP, C.POINTER(_I32)]),
    "xdtts_griffinlim_spsi_phase": (_I32, [_VP, _VP, _SZ, _VP, _VP]),
    "xdtts_griffinlim_spsi_phase_batch": (_I32, [_VP, _VP, _VP, _I32, _VP, _VP]),
    "xdtts_timbre_default": (None, [C.POINTER(Timbre)]),
    "xdtts_timbre_noise_bits": (_U32, [_U32, _U32, _U32]),
    "xdtts_griffinlim_set_timbre": (_I32, [_VP, C.POINTER(Timbre)]),
    "xdtts_griffinlim_get_timbre": (_I32, [_VP, C.POINTER(Timbre)]),
    "xdtts_griffinlim_timbre_linear": (_I32, [_VP, _VP, _SZ, C.POINTER(Timbre), _VP]),
    "xdtts_griffinlim_timbre_linear_batch": (_I32, [_VP, _VP, _VP, _I32, _VP, _VP]),
    "xdtts_denoise_default": (None, [C.POINTER(Denoise)]),
    "xdtts_griffinlim_set_denoise": (_I32, [_VP, C.POINTER(Denoise), _VP]),
    "xdtts_griffinlim_get_denoise": (_I32, [_VP, C.POINTER(Denoise), _VP, C.POINTER(_I32)]),
    "xdtts_griffinlim_last_denoise": (_I32, [_VP, _VP, _SZ, C.POINTER(_SZ)]),
    "xdtts_griffinlim_denoise_linear": (_I32, [_VP, _VP, _SZ, C.POINTER(Denoise), _VP, _VP]),
    "xdtts_griffinlim_denoise_linear_batch": (_I32, [_VP, _VP, _VP, _I32, _VP, _VP, _VP]),
    "xdtts_griffinlim_noise_profile": (_I32, [_VP, _VP, _SZ, _F, _VP]),
    "xdtts_denoise_rank": (_U32, [_SZ, _F]),
    "xdtts_denoise_floor": (_F, [_F]),
    "xdtts_denoise_tone": (_I32, [C.POINTER(Denoise), _VP]),
    "xdtts_denoise_reference": (_I32, [_VP, _SZ, C.POINTER(Denoise), _VP, _VP, C.POINTER(DenoiseStats)]),
    "xdtts_griffinlim_set_output_rate": (_I32, [_VP, _I32]),
    "xdtts_griffinlim_get_output_rate": (_I32, [_VP, C.POINTER(_I32)]),
    "xdtts_resample_plan": (_I32, [_I32, _SZ, C.POINTER(_I32), C.POINTER(_I32), C.POINTER(_I32), C.POINTER(_SZ)]),
    "xdtts_resample_filter": (_I32, [_I32, _VP, _SZ, C.POINTER(_SZ)]),
    "xdtts_griffinlim_resample": (_I32, [_VP, _VP, _SZ, _I32, _VP, C.POINTER(_SZ)]),
    "xdtts_griffinlim_resample_batch": (_I32, [_VP, _VP, _VP, _I32, _I32, _VP, _VP]),
    "xdtts_loudness_lufs": (C.c_double, [C.POINTER(Loudness)]),
    "xdtts_griffinlim_set_loudness": (_I32, [_VP, _F, _F]),
    "xdtts_griffinlim_get_loudness": (_I32, [_VP, _PF, _PF]),
    "xdtts_griffinlim_last_loudness": (_I32, [_VP, _VP, _SZ, C.POINTER(_SZ)]),
    "xdtts_griffinlim_loudness": (_I32, [_VP, _VP, _SZ, _I32, _VP]),
    "xdtts_griffinlim_loudness_batch": (_I32, [_VP, _VP, _VP, _I32, _I32, _VP]),
    "xdtts_stream_opts_default": (None, [C.POINTER(StreamOpts)]),
    "xdtts_stream_sample_bytes": (_SZ, [_I32]),
    "xdtts_stream_plan": (_I32, [_VP, _I32, _VP, _VP, C.POINTER(_SZ)]),
    "xdtts_stream_fade_table": (_I32, [_I32, _VP]),
    "xdtts_stream_encode_sample": (_I32, [_F, _I32, _I32, _U32, _SZ, _VP]),
    "xdtts_griffinlim_join": (_I32, [_VP, _VP, _VP, _I32, _VP, _I32, C.POINTER(StreamOpts), _VP, _SZ, _VP, C.POINTER(_SZ)]),
    "xdtts_synthesize_document": (_I32, [_VP, _VP, _VP, _VP, _VP, _VP, _I32, C.POINTER(InferOpts), _VP, _VP, C.POINTER(StreamOpts), _VP, _VP,
                                         C.POINTER(_VP), _VP, C.POINTER(_SZ)]),
    "xdtts_loudness_plan": (_I32, [_I32, _SZ, C.POINTER(_I32), C.POINTER(_SZ)]),
    "xdtts_loudness_filter": (_I32, [_I32, _VP]),
    "xdtts_true_peak_filter": (_I32, [_VP]),
    "xdtts_griffinlim_set_limiter": (_I32, [_VP, _I32]),
    "xdtts_griffinlim_get_limiter": (_I32, [_VP, C.POINTER(_I32)]),
    "xdtts_griffinlim_last_limiter": (_I32, [_VP, _VP, _SZ, C.POINTER(_SZ)]),
    "xdtts_griffinlim_limit": (_I32, [_VP, _VP, _SZ, _I32, C.c_double, C.c_double, _I32, _VP, _VP]),
    "xdtts_griffinlim_limit_batch": (_I32, [_VP, _VP, _VP, _I32, _I32, C.c_double, C.c_double, _I32, _VP, _VP]),
    "xdtts_limiter_plan": (_I32, [_I32, _I32, C.POINTER(_I32), C.POINTER(_I32)]),
    "xdtts_limiter_window": (_I32, [_I32, _I32, _VP]),
    "xdtts_limiter_reference": (_I32, [_VP, _SZ, _I32, C.c_double, C.c_double, _I32, _VP, _VP]),
    "xdtts_compressor_default": (None, [_VP]),
    "xdtts_compressor_preset": (_I32, [_I32, _VP]),
    "xdtts_griffinlim_set_compressor": (_I32, [_VP, _VP]),
    "xdtts_griffinlim_get_compressor": (_I32, [_VP, _VP, C.POINTER(_I32)]),
    "xdtts_griffinlim_last_compressor": (_I32, [_VP, _VP, _SZ, C.POINTER(_SZ)]),
    "xdtts_griffinlim_compress": (_I32, [_VP, _VP, _SZ, _I32, _VP, _VP, _VP]),
    "xdtts_griffinlim_compress_batch": (_I32, [_VP, _VP, _VP, _I32, _I32, _VP, _VP, _VP]),
    "xdtts_compressor_plan": (_I32, [_I32, _VP, C.POINTER(_I32), C.POINTER(_I32), C.POINTER(_I32), C.POINTER(_I32), C.POINTER(_I32)]),
    "xdtts_compressor_level": (_I32, [_VP, _SZ, _VP]),
    "xdtts_compressor_envelope": (_I32, [_VP, _SZ, _I32, _VP, _VP]),
    "xdtts_compressor_reference": (_I32, [_VP, _SZ, _I32, _VP, _VP, _VP]),
    "xdtts_silence_default": (None, [_VP]),
    "xdtts_griffinlim_set_silence": (_I32, [_VP, _VP]),
    "xdtts_griffinlim_get_silence": (_I32, [_VP, _VP, C.POINTER(_I32)]),
    "xdtts_griffinlim_last_silence": (_I32, [_VP, _VP, _SZ, C.POINTER(_SZ)]),
    "xdtts_griffinlim_trim": (_I32, [_VP, _VP, _SZ, _I32, _VP, _VP, _VP]),
    "xdtts_griffinlim_trim_batch": (_I32, [_VP, _VP, _VP, _I32, _I32, _VP, _VP, _VP]),
    "xdtts_silence_plan": (_I32, [_I32, _VP] + [C.POINTER(_I32)] * 6 + [C.POINTER(C.c_float)]),
    "xdtts_silence_keep": (_I32, [_VP, _SZ, _I32, _VP, _VP]),
    "xdtts_silence_reference": (_I32, [_VP, _SZ, _I32, _VP, _VP, _VP]),
    "xdtts_griffinlim_free": (None, [_VP]),
    "xdtts_synthesize_ids": (_I32, [_VP, _VP, _VP, _SZ, _VP, _SZ, C.POINTER(InferOpts), C.POINTER(_PF), C.POINTER(_SZ), C.POINTER(_PF), C.POINTER(_SZ)]),
    "xdtts_synthesize_ids_prosody": (_I32, [_VP, _VP, _VP, _SZ, _VP, _SZ, C.POINTER(InferOpts), C.POINTER(Prosody), C.POINTER(_PF), C.POINTER(_SZ), C.POINTER(_PF), C.POINTER(_SZ)]),
    "xdtts_synthesize_ids_contour": (_I32, [_VP, _VP, _VP, _SZ, _VP, _SZ, C.POINTER(InferOpts), C.POINTER(ProsodyContour), C.POINTER(_PF), C.POINTER(_SZ), C.POINTER(_PF), C.POINTER(_SZ)]),
    "xdtts_synthesize_ids_contour_at_ids": (_I32, [_VP, _VP, _VP, _SZ, _VP, _SZ, C.POINTER(InferOpts), C.POINTER(ProsodyContour), C.POINTER(_PF), C.POINTER(_SZ), C.POINTER(_PF), C.POINTER(_SZ)]),
    "xdtts_synthesize_batch_contour": (_I32, [_VP, _VP, _VP, _VP, _I32, _I32, _VP, _I32, C.POINTER(InferOpts), _VP, _VP, _VP, _VP, _VP, _VP]),
    "xdtts_synthesize_batch_contour_at_ids": (_I32, [_VP, _VP, _VP, _VP, _I32, _I32, _VP, _I32, C.POINTER(InferOpts), _VP, _VP, _VP, _VP, _VP, _VP]),
    "xdtts_synthesize_ids_pitch_target": (_I32, [_VP, _VP, _VP, _SZ, _VP, _SZ, C.POINTER(InferOpts), C.POINTER(F0Opts), C.POINTER(PitchTarget), C.POINTER(ProsodyContour), C.POINTER(_PF), C.POINTER(_SZ), C.POINTER(_PF), C.POINTER(_SZ)]),
    "xdtts_synthesize_batch_pitch_target": (_I32, [_VP, _VP, _VP, _VP, _I32, _I32, _VP, _I32, C.POINTER(InferOpts), _VP, C.POINTER(F0Opts), _VP, _VP, _VP, _VP, _VP, _VP]),
    "xdtts_synthesize_batch": (_I32, [_VP, _VP, _VP, _VP, _I32, _I32, _VP, _I32, C.POINTER(InferOpts), _VP, _VP, _VP, _VP, _VP]),
    "xdtts_synthesize_sequence": (_I32, [_VP, _VP, _VP, _VP, _VP, _VP, _I32, C.POINTER(InferOpts), _VP, _VP, _VP, _VP]),
    "xdtts_synthesize_batch_prosody": (_I32, [_VP, _VP, _VP, _VP, _I32, _I32, _VP, _I32, C.POINTER(InferOpts), _VP, _VP, _VP, _VP, _VP, _VP]),
    "xdtts_synthesize_sequence_prosody": (_I32, [_VP, _VP, _VP, _VP, _VP, _VP, _I32, C.POINTER(InferOpts), _VP, _VP, _VP, _VP, _VP]),
    "xdtts_symbol_count": (_I32, []),
    "xdtts_symbol_token": (C.c_char_p, [_I32]),
    "xdtts_unit_id": (C.c_int64, [C.c_char_p, _I32]),
    "xdtts_split_score": (_I32, [C.c_int64]),
    "xdtts_find_splits": (_I32, [_VP, _SZ, _SZ, _VP, _SZ, C.POINTER(_SZ)]),
    "xdtts_audio_to_i16": (_I32, [_VP, _SZ, _VP]),
    "xdtts_build_info": (C.c_char_p, []),
    "xdtts_edge_floor_us": (_I32, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double)]),
    "xdtts_default_device": (C.c_int32, []),
    "xdtts_silence_samples": (_SZ, [C.c_double, _U32]),
    "xdtts_silence_samples_duration": (_SZ, [C.c_uint64, _U32, _U32]),
    "xdtts_wav_write": (_I32, [C.c_char_p, _VP, _SZ, _U32]),
    "xdtts_npy_write_f32": (_I32, [C.c_char_p, _VP, _SZ, _SZ]),
    "xdtts_real_time_factor": (C.c_double, [C.c_double, _SZ]),
    "xdtts_free": (None, [_VP]),
    "xdtts_last_error": (C.c_char_p, []),
    "xdtts_device_count": (_I32, []),
}


def _share_torch_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64
    and ask for them by file name, so a process that loads libxdtts_hip.so first (system ROCm runtime,
    soname libamdhip64.so.7) and imports torch later ends up with TWO runtimes driving the same GPU
    (observed: a device-side error word the host never sees).  If torch is installed but not imported
    yet, map ITS runtime first -- without importing torch -- so that our DT_NEEDED resolves to that copy
    and a later `import torch` finds it already loaded.  With torch imported first nothing is needed;
    without torch installed the system runtime is the only one."""
    import importlib.util
    import sys

    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if not spec or not spec.origin:
        return
    lib = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(lib):
        try:
            C.CDLL(lib, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def _load():
    _share_torch_hip_runtime()
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s not found: build it with `make -C %s` (or __graft_entry__.build()); there is no CPU fallback" % (LIB_PATH, _HERE)
        )
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


def _check(status):
    if status != 0:
        raise XdttsError(status, lib.xdtts_last_error().decode("utf-8", "replace"))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _prosody_array(prosody, n):
    """A list of n Prosody -> the C array xdtts_prosody[n] the batch and sequence entries take."""
    ps = list(prosody)
    if len(ps) != n:
        raise ValueError("prosody= takes one Prosody per utterance: %d for %d utterances" % (len(ps), n))
    return (Prosody * n)(*ps)


def _contour_array(contour, n):
    """A list of n ProsodyContour -> the C array xdtts_prosody_contour[n] the batch entries take."""
    cs = list(contour)
    if len(cs) != n:
        raise ValueError("contour= takes one ProsodyContour per utterance: %d for %d utterances" % (len(cs), n))
    arr = (ProsodyContour * n)()
    for u, c in enumerate(cs):
        arr[u].points, arr[u].n_points, arr[u].lifter, arr[u].log_floor = c.points, c.n_points, c.lifter, c.log_floor
    arr._keep = cs  # the point arrays
    return arr


def _target_arrays(targets, contours, n):
    """n PitchTarget (and n ProsodyContour or None each, or None for none at all) -> the C arrays the target entries take:
    xdtts_pitch_target[n] and an array of n contour pointers.  The third value keeps the contours alive."""
    ts = list(targets)
    if len(ts) != n:
        raise ValueError("target= takes one PitchTarget per utterance: %d for %d utterances" % (len(ts), n))
    ta = (PitchTarget * n)()
    for u, t in enumerate(ts):
        ta[u].mode, ta[u].value, ta[u].range = t.mode, t.value, t.range
    if contours is None:
        return ta, None, None
    cs = list(contours)
    if len(cs) != n:
        raise ValueError("contour= takes one ProsodyContour (or None) per utterance: %d for %d utterances" % (len(cs), n))
    ca = (C.c_void_p * n)(*[(None if c is None else C.addressof(c)) for c in cs])
    return ta, ca, cs


def _opt_ref(x):
    return None if x is None else C.byref(x)


def _one_of(prosody, contour):
    if prosody is not None and contour is not None:
        raise ValueError("pass prosody= or contour=, not both")


def default_opts(**kw):
    """xdtts_infer_opts with the reference's defaults; `dropout_masks=` takes a uint8 array (chunks, steps, 2, 256) of keep
    bytes and selects dropout_mode 2 (the array is kept alive by the returned struct)."""
    o = InferOpts()
    lib.xdtts_infer_opts_default(C.byref(o))
    masks = kw.pop("dropout_masks", None)
    for k, v in kw.items():
        setattr(o, k, v)
    if masks is not None:
        m = np.ascontiguousarray(masks, dtype=np.uint8)
        if m.ndim != 4 or m.shape[2:] != (2, 256):
            raise ValueError("dropout_masks must be (chunks, steps, 2, 256)")
        o._masks_keepalive = m
        o.dropout_masks = m.ctypes.data
        o.dropout_mask_steps = m.shape[1]
        o.dropout_mode = 2
    return o


def device_count():
    return lib.xdtts_device_count()


def tensor_table():
    out = []
    for i in range(lib.xdtts_tensor_count()):
        shape = tuple(lib.xdtts_tensor_dim(i, d) for d in range(lib.xdtts_tensor_ndim(i)))
        out.append((lib.xdtts_tensor_name(i).decode(), shape, lib.xdtts_tensor_offset(i)))
    return out


def read_model_dir(path):
    """The host half of Tacotron2::load(path): the reference's model directory (encoder.onnx,
    decoder_iter.onnx, postnet.onnx -- src/tacotron2/mod.rs:246-259) or a tacotron2.xdtw container as a
    dict name -> array of the canonical tensors.  Needs no device."""
    blob = np.empty(lib.xdtts_tensor_total(), dtype=np.float32)
    _check(lib.xdtts_model_dir_read(os.fsencode(path), _ptr(blob), blob.size))
    return {n: blob[off : off + int(np.prod(shape))].reshape(shape) for n, shape, off in tensor_table()}


def describe_model_dir(path):
    """{file: (inputs, outputs)} of the three ONNX graphs of a model directory -- the names the reference binds at
    src/tacotron2/mod.rs:284-296,306-307,332-339,349."""
    need = C.c_size_t()
    _check(lib.xdtts_model_dir_describe(os.fsencode(path), None, 0, C.byref(need)))
    buf = C.create_string_buffer(need.value)
    _check(lib.xdtts_model_dir_describe(os.fsencode(path), buf, need.value, None))
    out = {}
    for line in buf.value.decode().splitlines():
        f, rest = line.split(": inputs ", 1)
        i, o = rest.split(" ; outputs ", 1)
        out[f] = ([x for x in i.split(",") if x], [x for x in o.split(",") if x])
    return out


class _Pinned:
    """Owner of one library buffer (pinned host memory): xdtts_free when the last view of it goes."""

    def __init__(self, addr):
        self.addr = addr

    def __del__(self):
        if self.addr and lib is not None:
            lib.xdtts_free(C.cast(self.addr, _PF))
            self.addr = None


def _take(ptr, n, shape):
    """A numpy view of a library-owned pinned buffer (no copy: a batch of audio is tens of MB); the buffer
    goes back to the library's pool when the array and every view of it are gone."""
    addr = C.cast(ptr, C.c_void_p).value
    if not n or not addr:
        if addr:
            lib.xdtts_free(ptr)
        return np.zeros(shape, dtype=np.float32)
    buf = (C.c_float * int(n)).from_address(addr)
    buf._owner = _Pinned(addr)  # numpy keeps `buf` as the array's base, `buf` keeps the owner
    return np.frombuffer(buf, dtype=np.float32).reshape(shape)


def generate_id_list():
    """generate_id_list() -- src/tacotron2/mod.rs:90-122, as token strings."""
    return [lib.xdtts_symbol_token(i).decode() for i in range(lib.xdtts_symbol_count())]


def unit_id(token, as_character=False):
    """Unit::from_str + best_match_for_unit (src/phonemes.rs:450-487,627-660); None if no id."""
    i = lib.xdtts_unit_id(token.encode(), 1 if as_character else 0)
    return None if i < 0 else int(i)


def units_to_ids(tokens, as_character=False):
    """The filter_map of src/tacotron2/mod.rs:403-406: units without an id are dropped."""
    out = [unit_id(t, as_character) for t in tokens]
    return np.array([i for i in out if i is not None], dtype=np.int64)


SAMPLE_RATE = 22050  # WAV_SPEC, src/lib.rs:25-30


def build_info():
    """xdtts_build_info() as a dict (src_sha256, arch, built_utc, compiler)."""
    return dict(kv.split("=", 1) for kv in lib.xdtts_build_info().decode().split(" ") if "=" in kv)


def source_hash():
    """The hash the Makefile computes: sha256 over csrc/* and include/xdtts.h in name order."""
    import glob
    import hashlib

    here = os.path.dirname(os.path.abspath(__file__))
    files = sorted(glob.glob(os.path.join(here, "csrc", "*")) + [os.path.join(here, "..", "include", "xdtts.h")],
                   key=lambda p: os.path.relpath(p, here))
    h = hashlib.sha256()
    for f in files:
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


DEVICE_DEFAULT = -1  # XDTTS_DEVICE_DEFAULT: the process's default GPU (environment variable XDTTS_DEVICE, 0 without it)


def default_device():
    """What device_id = DEVICE_DEFAULT resolves to now (xdtts_default_device)."""
    v = lib.xdtts_default_device()
    if v < 0:
        raise XdttsError(2, lib.xdtts_last_error().decode())
    return int(v)


def edge_floor_us(device_id=0, steps=2000, T=100, tuned=True):
    """Latency floor of one persistent-decoder step on this device now (xdtts_edge_floor_us): us per step."""
    us = C.c_double()
    _check(lib.xdtts_edge_floor_us(device_id, steps, T, 1 if tuned else 0, C.byref(us)))
    return us.value


def audio_to_i16(audio):
    """`(sample * i16::MAX as f32) as i16` (src/lib.rs:153-155): truncating, saturating, NaN -> 0."""
    a = np.ascontiguousarray(audio, dtype=np.float32).ravel()
    out = np.empty(a.size, dtype=np.int16)
    _check(lib.xdtts_audio_to_i16(_ptr(a), a.size, _ptr(out)))
    return out


def silence_samples(seconds, sample_rate=SAMPLE_RATE):
    """write_silence (src/lib.rs:162-176)."""
    return int(lib.xdtts_silence_samples(float(seconds), int(sample_rate)))


def silence_samples_duration(secs, nanos, sample_rate=SAMPLE_RATE):
    """write_silence (src/lib.rs:162-176) from a Rust Duration's (secs, subsec_nanos): f32 throughout."""
    return int(lib.xdtts_silence_samples_duration(int(secs), int(nanos), int(sample_rate)))


def write_wav(path, audio, sample_rate=SAMPLE_RATE):
    """f32 audio (or ready int16 PCM) -> mono 16-bit WAV with the reference's WAV_SPEC."""
    pcm = np.ascontiguousarray(audio) if np.asarray(audio).dtype == np.int16 else audio_to_i16(audio)
    _check(lib.xdtts_wav_write(os.fsencode(path), _ptr(pcm), pcm.size, int(sample_rate)))


def write_mel_npy(path, mel):
    """ndarray_npy::write_npy of the (80, F) spectrogram (src/lib.rs:128-141)."""
    m = np.ascontiguousarray(mel, dtype=np.float32)
    _check(lib.xdtts_npy_write_f32(os.fsencode(path), _ptr(m), m.shape[0], m.shape[1]))


def real_time_factor(compute_seconds, n_samples):
    return float(lib.xdtts_real_time_factor(float(compute_seconds), int(n_samples)))


def find_splits(ids, max_size=100):
    """find_splits(units, max_size) -- src/phonemes.rs:681-753."""
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    out = np.empty(max(ids.size, 1) + 2, dtype=np.uintp)
    n = C.c_size_t()
    _check(lib.xdtts_find_splits(_ptr(ids), ids.size, max_size, _ptr(out), out.size, C.byref(n)))
    return out[: n.value].astype(np.int64)


class Tacotron2:
    """Mirror of ``Tacotron2`` (src/tacotron2/mod.rs:139-148): ``load`` then ``infer``."""

    def __init__(self, handle):
        self._h = handle

    # -- constructors ---------------------------------------------------------------------------
    @classmethod
    def load(cls, path, device_id=0):
        """Tacotron2::load(path) -- src/tacotron2/mod.rs:242."""
        h = C.c_void_p()
        _check(lib.xdtts_tacotron2_load(os.fsencode(path), device_id, C.byref(h)))
        return cls(h)

    @classmethod
    def synthetic(cls, seed=20240327, rec_scale=1.0, device_id=0):
        h = C.c_void_p()
        _check(lib.xdtts_tacotron2_load_synthetic(seed, rec_scale, device_id, C.byref(h)))
        return cls(h)

    @classmethod
    def from_blob(cls, blob, device_id=0):
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        h = C.c_void_p()
        _check(lib.xdtts_tacotron2_load_blob(_ptr(blob), blob.size, device_id, C.byref(h)))
        return cls(h)

    def close(self):
        if self._h:
            lib.xdtts_tacotron2_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def save(self, path):
        _check(lib.xdtts_tacotron2_save(self._h, os.fsencode(path)))

    def blob(self):
        """The canonical flat fp32 weight blob of this handle (what from_blob / xdtts_tacotron2_load_blob take)."""
        out = np.zeros(lib.xdtts_tensor_total(), dtype=np.float32)
        for i, (_n, shape, off) in enumerate(tensor_table()):
            t = np.empty(shape, dtype=np.float32)
            _check(lib.xdtts_tacotron2_get_tensor(self._h, i, _ptr(t)))
            out[off : off + t.size] = t.ravel()
        return out

    def get_tensor(self, name):
        for i, (n, shape, _off) in enumerate(tensor_table()):
            if n == name:
                out = np.empty(shape, dtype=np.float32)
                _check(lib.xdtts_tacotron2_get_tensor(self._h, i, _ptr(out)))
                return out
        raise KeyError(name)

    # -- the reference surface --------------------------------------------------------------------
    def infer(self, ids, splits=None, opts=None):
        """Tacotron2::infer -- src/tacotron2/mod.rs:398; ids after best_match_for_unit, splits from
        find_splits.  Returns the (80, F) mel like the reference's Array2<f32>."""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        sp = None if splits is None else np.ascontiguousarray(splits, dtype=np.uintp)
        mel, nf = _PF(), C.c_size_t()
        _check(
            lib.xdtts_tacotron2_infer_ids(
                self._h, _ptr(ids), ids.size, None if sp is None else _ptr(sp), 0 if sp is None else sp.size, C.byref(opts) if opts else None, C.byref(mel), C.byref(nf)
            )
        )
        return _take(mel, N_MEL * nf.value, (N_MEL, nf.value))

    def infer_units(self, tokens, opts=None, as_character=False):
        """Tacotron2::infer(&[Unit]) end to end (mod.rs:398-437): unit tokens -> ids (units with no
        id dropped) -> find_splits(.., window) -> chunks -> mel."""
        ids = units_to_ids(tokens, as_character)
        window = opts.max_chunk if opts else 100
        return self.infer(ids, splits=find_splits(ids, window), opts=opts)

    def infer_batch(self, ids_list, opts=None, fixed_steps=None):
        """B independent chunks (infer_chunk, mod.rs:361-393) decoded in lock-step."""
        B = len(ids_list)
        lens = np.array([len(x) for x in ids_list], dtype=np.int32)
        stride = int(lens.max()) if B else 1
        ids = np.zeros((B, stride), dtype=np.int64)
        for b, x in enumerate(ids_list):
            ids[b, : len(x)] = x
        fs = None if fixed_steps is None else np.ascontiguousarray(fixed_steps, dtype=np.int32)
        mels = (_PF * B)()
        nf = (C.c_size_t * B)()
        _check(lib.xdtts_tacotron2_infer_batch(self._h, _ptr(ids), _ptr(lens), B, stride, C.byref(opts) if opts else None, None if fs is None else _ptr(fs), mels, nf))
        return [_take(mels[b], N_MEL * nf[b], (N_MEL, nf[b])) for b in range(B)]

    # -- parity hooks: the three graphs one at a time ---------------------------------------------
    def encoder(self, ids):
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        T = ids.size
        memory = np.empty((T, EMB), dtype=np.float32)
        pmem = np.empty((T, ATT_DIM), dtype=np.float32)
        _check(lib.xdtts_tacotron2_encoder(self._h, _ptr(ids), T, _ptr(memory), _ptr(pmem)))
        return memory, pmem

    BILSTM_ENGINES = {None: -1, "single": 0, "cooperative": 1}

    def encoder_batch(self, ids, engine=None):
        """encoder.onnx for B chunks at once, the way a batch request runs it: ids (B, T) zero-padded -> memory (B, T, 512),
        processed_memory (B, T, 128).  engine: None (the handle's), "cooperative" or "single" (the BiLSTM recurrence)."""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        B, T = ids.shape
        memory = np.empty((B, T, EMB), dtype=np.float32)
        pmem = np.empty((B, T, ATT_DIM), dtype=np.float32)
        _check(lib.xdtts_tacotron2_encoder_batch(self._h, self.BILSTM_ENGINES[engine], _ptr(ids), B, T, _ptr(memory), _ptr(pmem)))
        return memory, pmem

    def decoder(self, memory, pmem, n_valid, opts=None):
        memory = np.ascontiguousarray(memory, dtype=np.float32)
        pmem = np.ascontiguousarray(pmem, dtype=np.float32)
        o = opts if opts else default_opts()
        frames = np.empty((o.max_steps, N_MEL), dtype=np.float32)
        gates = np.empty(o.max_steps, dtype=np.float32)
        nf = C.c_size_t()
        _check(lib.xdtts_tacotron2_decoder(self._h, _ptr(memory), _ptr(pmem), memory.shape[0], n_valid, C.byref(o), _ptr(frames), _ptr(gates), C.byref(nf)))
        return frames[: nf.value].copy(), gates[: nf.value].copy()

    def decoder_step(self, memory, pmem, n_valid, state, decoder_input, step, opts=None):
        """ONE decoder_iter call (mod.rs:304).  `state` = dict with the reference's tensor names
        (attention_hidden, attention_cell, decoder_hidden, decoder_cell, attention_weights,
        attention_weights_cum, attention_context); returns (decoder_output, gate_prediction, new state)."""
        memory = np.ascontiguousarray(memory, dtype=np.float32)
        pmem = np.ascontiguousarray(pmem, dtype=np.float32)
        names = ("attention_hidden", "attention_cell", "decoder_hidden", "decoder_cell", "attention_weights", "attention_weights_cum", "attention_context")
        st = {k: np.array(state[k], dtype=np.float32, order="C") for k in names}
        din = np.ascontiguousarray(decoder_input, dtype=np.float32)
        out, gate = np.empty(N_MEL, dtype=np.float32), np.empty(1, dtype=np.float32)
        _check(lib.xdtts_tacotron2_decoder_step(self._h, _ptr(memory), _ptr(pmem), memory.shape[0], n_valid, C.byref(opts) if opts else None, step,
                                                _ptr(din), *[_ptr(st[k]) for k in names], _ptr(out), _ptr(gate)))
        return out, float(gate[0]), st

    ENGINES = {"launch": 0, "persistent": 1, "batched": 2, "persistent8": 3}

    def decoder_steps(self, engine, memory, pmem, n_valid, states, decoder_input, step0, n_steps=1, opts=None):
        """n_steps decoder_iter calls for B chunks through the named engine ("launch" / "persistent" / "batched").
        memory (B, T, 512), pmem (B, T, 128), n_valid (B,), decoder_input (B, 80); `states` = dict of (B, ...) arrays with the
        reference's tensor names.  Returns (decoder_output (B, n_steps, 80), gate_prediction (B, n_steps), new states)."""
        memory = np.ascontiguousarray(memory, dtype=np.float32)
        pmem = np.ascontiguousarray(pmem, dtype=np.float32)
        B, T = memory.shape[0], memory.shape[1]
        nv = np.ascontiguousarray(n_valid, dtype=np.int32)
        names = ("attention_hidden", "attention_cell", "decoder_hidden", "decoder_cell", "attention_weights", "attention_weights_cum", "attention_context")
        st = {k: np.array(states[k], dtype=np.float32, order="C") for k in names}
        din = np.ascontiguousarray(decoder_input, dtype=np.float32)
        out, gate = np.empty((B, n_steps, N_MEL), dtype=np.float32), np.empty((B, n_steps), dtype=np.float32)
        _check(lib.xdtts_tacotron2_decoder_steps(self._h, self.ENGINES[engine], B, _ptr(memory), _ptr(pmem), T, _ptr(nv), C.byref(opts) if opts else None,
                                                 step0, n_steps, _ptr(din), *[_ptr(st[k]) for k in names], _ptr(out), _ptr(gate)))
        return out, gate, st

    def engine_state(self):
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        _check(lib.xdtts_tacotron2_engine_state(self._h, C.byref(a), C.byref(b), C.byref(c)))
        e = C.c_int32()
        _check(lib.xdtts_tacotron2_small_batch_engine_state(self._h, C.byref(e)))
        return {"decoder_persistent": a.value, "encoder_cooperative": b.value, "batched_attention": c.value, "decoder_persistent8": e.value}

    def engine_reset(self):
        _check(lib.xdtts_tacotron2_engine_reset(self._h))

    def postnet(self, frames):
        frames = np.ascontiguousarray(frames, dtype=np.float32)
        F = frames.shape[0]
        out = np.empty((N_MEL, F), dtype=np.float32)
        _check(lib.xdtts_tacotron2_postnet(self._h, _ptr(frames), F, _ptr(out)))
        return out

    def postnet_batch(self, frames_list, per_chunk=False):
        """postnet.onnx for n chunks through the group loop of a batch request: frames_list[i] is (F_i, 80).  Returns the
        (80, sum F) matrix with the chunks side by side, or with per_chunk the list of dense (80, F_i) matrices."""
        n = len(frames_list)
        F = np.array([np.shape(f)[0] for f in frames_list], dtype=np.int32)
        stride = int(F.max()) * N_MEL
        buf = np.zeros((n, stride), dtype=np.float32)
        for i, f in enumerate(frames_list):
            buf[i, : F[i] * N_MEL] = np.asarray(f, dtype=np.float32).reshape(-1)
        total = int(F.sum())
        out = np.empty(N_MEL * total, dtype=np.float32)
        _check(lib.xdtts_tacotron2_postnet_batch(self._h, _ptr(buf), stride, _ptr(F), n, 1 if per_chunk else 0, _ptr(out)))
        if not per_chunk:
            return out.reshape(N_MEL, total)
        ends = np.cumsum(F) * N_MEL
        return [out[e - F[i] * N_MEL:e].reshape(N_MEL, F[i]) for i, e in enumerate(ends)]

    def last_timings(self):
        ms = (C.c_float * 4)()
        steps = C.c_int32()
        _check(lib.xdtts_tacotron2_last_timings(self._h, C.byref(ms), C.byref(steps)))
        return {"encoder_ms": ms[0], "decoder_ms": ms[1], "postnet_ms": ms[2], "total_ms": ms[3], "steps": steps.value}

    # -- durations (include/xdtts.h: per-id durations and timing marks from the cumulative attention) ------------
    def set_durations(self, opts=None, **kw):
        """The durations setting: a DurationsOpts, or its fields as keywords (set_durations(on=1)); nothing = the default (off)."""
        o = opts if opts is not None else DurationsOpts(**kw)
        _check(lib.xdtts_tacotron2_set_durations(self._h, C.byref(o)))

    def get_durations(self):
        o = DurationsOpts()
        _check(lib.xdtts_tacotron2_get_durations(self._h, C.byref(o)))
        return o

    def last_durations_count(self):
        n = C.c_size_t()
        _check(lib.xdtts_tacotron2_last_durations_count(self._h, C.byref(n)))
        return n.value

    def last_durations(self, utterance=0):
        """(dur fp32, dur_q16 uint32, start_q16 uint64) of one utterance of the last call, one entry per id."""
        n = C.c_size_t()
        _check(lib.xdtts_tacotron2_last_durations(self._h, utterance, None, None, None, 0, C.byref(n)))
        dur, q, st = np.empty(n.value, dtype=np.float32), np.empty(n.value, dtype=np.uint32), np.empty(n.value, dtype=np.uint64)
        _check(lib.xdtts_tacotron2_last_durations(self._h, utterance, _ptr(dur), _ptr(q), _ptr(st), n.value, C.byref(n)))
        return dur, q, st

    def last_alignment(self, utterance=0):
        s = AlignmentStats()
        _check(lib.xdtts_tacotron2_last_alignment(self._h, utterance, C.byref(s)))
        return s

    def durations_gather(self, cum_a, cum_b, nframes, n_valid, order=None, batched=False, utt_of_chunk=None, opts=None):
        """Parity hook: the stage alone on caller arrays (cum_a / cum_b: (B, T) by slot).  (dur, dur_q16, start_q16, [stats])."""
        return _durations_call(lib.xdtts_tacotron2_durations_gather, (self._h,), cum_a, cum_b, nframes, n_valid, order, batched, utt_of_chunk, opts)


def _durations_call(fn, head, cum_a, cum_b, nframes, n_valid, order, batched, utt_of_chunk, opts):
    cum_a = np.ascontiguousarray(cum_a, dtype=np.float32)
    B, T = cum_a.shape
    cum_b = None if cum_b is None else np.ascontiguousarray(cum_b, dtype=np.float32)
    i32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)
    nframes, n_valid, order, utt_of_chunk = i32(nframes), i32(n_valid), i32(order), i32(utt_of_chunk)
    p = lambda a: None if a is None else _ptr(a)
    N, U = int(np.clip(n_valid, 0, T).sum()), B
    dur, q, st = np.empty(N, dtype=np.float32), np.empty(N, dtype=np.uint32), np.empty(N, dtype=np.uint64)
    stats = (AlignmentStats * max(U, 1))()
    n_ids, n_utt = C.c_size_t(), C.c_size_t()
    _check(fn(*head, p(cum_a), p(cum_b), B, T, p(nframes), p(n_valid), p(order), 1 if batched else 0, p(utt_of_chunk),
              C.byref(opts) if opts is not None else None, p(dur), p(q), p(st), N, stats, U, C.byref(n_ids), C.byref(n_utt)))
    return dur[:n_ids.value], q[:n_ids.value], st[:n_ids.value], [stats[u] for u in range(n_utt.value)]


def durations_reference(cum_a, cum_b, nframes, n_valid, order=None, batched=False, utt_of_chunk=None, opts=None):
    """xdtts_durations_reference: the durations stage on the host, serially (no device)."""
    return _durations_call(lib.xdtts_durations_reference, (), cum_a, cum_b, nframes, n_valid, order, batched, utt_of_chunk, opts)


def durations_position(start_q16, dur_q16, n_frames, x):
    """xdtts_durations_position: a position in ids -> a contour point's pos."""
    st, q = np.ascontiguousarray(start_q16, dtype=np.uint64), np.ascontiguousarray(dur_q16, dtype=np.uint32)
    return lib.xdtts_durations_position(_ptr(st), _ptr(q), st.size, n_frames, float(x))


def durations_samples(start_q16, hop=256, rate_out=22050):
    return lib.xdtts_durations_samples(int(start_q16), hop, rate_out)


def create_mel_filter_bank(sample_rate, n_fft, n_mels, fmin, fmax=None):
    """griffin_lim::mel::create_mel_filter_bank -- src/tacotron2/mod.rs:453 (fmax: Option<f32>)."""
    out = np.empty((n_mels, n_fft // 2 + 1), dtype=np.float32)
    _check(lib.xdtts_mel_filter_bank(sample_rate, n_fft, n_mels, fmin, float("nan") if fmax is None else fmax, _ptr(out)))
    return out


class GriffinLim:
    """Mirror of griffin_lim::GriffinLim: ``new(mel_basis, noverlap, power, iter, momentum)``
    (src/tacotron2/mod.rs:456) and ``infer(&mel)`` (src/lib.rs:141)."""

    def __init__(self, mel_basis, noverlap, power, iters, momentum, device_id=0, seed=0):
        basis = np.ascontiguousarray(mel_basis, dtype=np.float32)
        self._h = C.c_void_p()
        _check(lib.xdtts_griffinlim_new(_ptr(basis), basis.shape[0], basis.shape[1], noverlap, power, iters, momentum, device_id, C.byref(self._h)))
        self.n_mels, self.n_bins = basis.shape
        self.set_seed(seed)

    def set_seed(self, seed):
        _check(lib.xdtts_griffinlim_set_seed(self._h, seed))

    def set_opts(self, **kw):
        """nnls_iters, power_mode (0 inverse / 1 direct / 2 none), mel_decompress (0 exp / 1 none / 2 10^x),
        output_normalise (0 none / 1 peak / 2 rms / 3 rms limited to a peak of 1), rms_target, batch_shape (0 auto / 4 the single-utterance shape: bit-identical batches); unspecified
        fields keep their current value."""
        o = self.get_opts()
        for k, v in kw.items():
            setattr(o, k, v)
        _check(lib.xdtts_griffinlim_set_opts(self._h, C.byref(o)))

    def get_opts(self):
        o = GriffinLimOpts()
        _check(lib.xdtts_griffinlim_get_opts(self._h, C.byref(o)))
        return o

    def close(self):
        if self._h:
            lib.xdtts_griffinlim_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def infer(self, mel):
        mel = np.ascontiguousarray(mel, dtype=np.float32)
        audio, n = _PF(), C.c_size_t()
        _check(lib.xdtts_griffinlim_infer(self._h, _ptr(mel), mel.shape[0], mel.shape[1], C.byref(audio), C.byref(n)))
        return _take(audio, n.value, (n.value,))

    def infer_batch(self, mels, prosody=None, contour=None):
        """GriffinLim::infer for a list of (80, F_u) mels in one call; returns the list of audios.  prosody= (a list of one
        Prosody per utterance) runs the rate / pitch stage as one ragged launch behind the batch's mel -> linear
        (xdtts_griffinlim_infer_batch_prosody): audio u has 256 * (prosody_frames(F_u, rate_u) - 1) samples.  contour= (a list of
        one ProsodyContour per utterance) runs the contour stage there instead (xdtts_griffinlim_infer_batch_contour)."""
        _one_of(prosody, contour)
        ms = [np.ascontiguousarray(m, dtype=np.float32) for m in mels]
        n = len(ms)
        ptrs = (C.c_void_p * n)(*[m.ctypes.data for m in ms])
        nf = (C.c_size_t * n)(*[m.shape[1] for m in ms])
        audios = (_PF * n)()
        ns = (C.c_size_t * n)()
        if contour is not None:
            _check(lib.xdtts_griffinlim_infer_batch_contour(self._h, ptrs, ms[0].shape[0], nf, n, _contour_array(contour, n), audios, ns))
        elif prosody is None:
            _check(lib.xdtts_griffinlim_infer_batch(self._h, ptrs, ms[0].shape[0], nf, n, audios, ns))
        else:
            _check(lib.xdtts_griffinlim_infer_batch_prosody(self._h, ptrs, ms[0].shape[0], nf, n, _prosody_array(prosody, n), audios, ns))
        return [_take(audios[u], ns[u], (ns[u],)) for u in range(n)]

    def batch_plan(self, n_frames):
        """xdtts_griffinlim_batch_plan (host arithmetic, nothing is launched): how infer_batch would pack utterances of these
        frame counts into persistent launches if called now -- {"TF", "WG", "n_launches", "launch_of" (per utterance, -1 =
        alone), "n_cu" (0: no usable persistent engine), "per_cu4"}; reads batch_shape, XDTTS_GL and XDTTS_GL_BATCH_FORCE."""
        n = len(n_frames)
        nf = (C.c_size_t * max(n, 1))(*[int(F) for F in n_frames])
        of = (C.c_int32 * max(n, 1))()
        v = [C.c_int32() for _ in range(5)]
        _check(lib.xdtts_griffinlim_batch_plan(self._h, nf, n, C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), of, C.byref(v[3]), C.byref(v[4])))
        return {"TF": v[0].value, "WG": v[1].value, "n_launches": v[2].value, "launch_of": [of[u] for u in range(n)],
                "n_cu": v[3].value, "per_cu4": v[4].value}

    def infer_linear(self, S, phase0=None, iters=0):
        S = np.ascontiguousarray(S, dtype=np.float32)
        p0 = None if phase0 is None else np.ascontiguousarray(phase0, dtype=np.float32)
        audio, n = _PF(), C.c_size_t()
        _check(lib.xdtts_griffinlim_infer_linear(self._h, _ptr(S), None if p0 is None else _ptr(p0), S.shape[1], iters, C.byref(audio), C.byref(n)))
        return _take(audio, n.value, (n.value,))

    def step(self, S, angles, rebuilt, n_iter=1):
        """Parity hook: n_iter iterations from the state (angles, rebuilt), both (n_bins, F, 2); returns
        the new (angles, rebuilt)."""
        S = np.ascontiguousarray(S, dtype=np.float32)
        a = np.array(angles, dtype=np.float32, order="C")
        r = np.array(rebuilt, dtype=np.float32, order="C")
        _check(lib.xdtts_griffinlim_step(self._h, _ptr(S), _ptr(a), _ptr(r), S.shape[1], n_iter))
        return a, r

    def mel_to_linear(self, mel):
        mel = np.ascontiguousarray(mel, dtype=np.float32)
        S = np.empty((self.n_bins, mel.shape[1]), dtype=np.float32)
        _check(lib.xdtts_griffinlim_mel_to_linear(self._h, _ptr(mel), mel.shape[0], mel.shape[1], _ptr(S)))
        return S

    def last_timings(self):
        """(after infer_prosody / synthesize(prosody=...): mel_to_linear_ms covers mel -> linear and the prosody stage; with
        phase_init 1 the SPSI stage too; after prosody_linear / spsi_phase it is the stage alone)"""
        ms = (C.c_float * 3)()
        _check(lib.xdtts_griffinlim_last_timings(self._h, C.byref(ms)))
        return {"mel_to_linear_ms": ms[0], "iterations_ms": ms[1], "total_ms": ms[2]}

    # -- prosody: speaking rate and pitch on the magnitude, between mel -> linear and the loop ----
    def prosody_linear(self, S, prosody):
        """The prosody stage alone (parity hook): S (n_bins, F) -> S' (n_bins, F'), F' = prosody_frames(F, prosody.rate)."""
        S = np.ascontiguousarray(S, dtype=np.float32)
        Fp = prosody_frames(S.shape[1], prosody.rate)
        out = np.empty((self.n_bins, max(Fp, 1)), dtype=np.float32)
        nf = C.c_size_t()
        _check(lib.xdtts_griffinlim_prosody_linear(self._h, _ptr(S), S.shape[1], C.byref(prosody), _ptr(out), C.byref(nf)))
        assert nf.value == Fp
        return out

    def prosody_linear_batch(self, S_list, prosody_list):
        """The ragged stage alone (parity hook): a list of S_u (n_bins, F_u) and one Prosody each -> the list of S'_u
        (n_bins, F'_u), one k_prosody_batch launch for all of them."""
        Ss = [np.ascontiguousarray(S, dtype=np.float32) for S in S_list]
        n = len(Ss)
        pa = _prosody_array(prosody_list, n)
        Fp = [prosody_frames(S.shape[1], p.rate) for S, p in zip(Ss, pa)]
        outs = [np.empty((self.n_bins, max(f, 1)), dtype=np.float32) for f in Fp]
        sp = (C.c_void_p * n)(*[S.ctypes.data for S in Ss])
        op = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        nf = (C.c_size_t * n)(*[S.shape[1] for S in Ss])
        nfo = (C.c_size_t * n)()
        _check(lib.xdtts_griffinlim_prosody_linear_batch(self._h, sp, nf, n, pa, op, nfo))
        assert list(nfo) == Fp
        return outs

    def infer_prosody(self, mel, prosody):
        """infer() with the prosody stage behind mel -> linear: 256 * (F' - 1) samples."""
        mel = np.ascontiguousarray(mel, dtype=np.float32)
        audio, n = _PF(), C.c_size_t()
        _check(lib.xdtts_griffinlim_infer_prosody(self._h, _ptr(mel), mel.shape[0], mel.shape[1], C.byref(prosody), C.byref(audio), C.byref(n)))
        return _take(audio, n.value, (n.value,))

    # -- prosody contours: rate, pitch and gain that vary inside an utterance ----
    def contour_linear(self, S, contour):
        """The contour stage alone (parity hook): S (n_bins, F) -> S' (n_bins, F'), F' = prosody_contour_frames(contour, F)."""
        S = np.ascontiguousarray(S, dtype=np.float32)
        Fp = prosody_contour_frames(contour, S.shape[1])
        out = np.empty((self.n_bins, max(Fp, 1)), dtype=np.float32)
        nf = C.c_size_t()
        _check(lib.xdtts_griffinlim_contour_linear(self._h, _ptr(S), S.shape[1], C.byref(contour), _ptr(out), C.byref(nf)))
        assert nf.value == Fp
        return out

    def contour_linear_batch(self, S_list, contour_list):
        """The ragged contour stage alone (parity hook): a list of S_u (n_bins, F_u) and one ProsodyContour each -> the list of
        S'_u (n_bins, F'_u), one k_prosody_contour launch for all of them."""
        Ss = [np.ascontiguousarray(S, dtype=np.float32) for S in S_list]
        n = len(Ss)
        ca = _contour_array(contour_list, n)
        Fp = [prosody_contour_frames(c, S.shape[1]) for S, c in zip(Ss, contour_list)]
        outs = [np.empty((self.n_bins, max(f, 1)), dtype=np.float32) for f in Fp]
        sp = (C.c_void_p * n)(*[S.ctypes.data for S in Ss])
        op = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        nf = (C.c_size_t * n)(*[S.shape[1] for S in Ss])
        nfo = (C.c_size_t * n)()
        _check(lib.xdtts_griffinlim_contour_linear_batch(self._h, sp, nf, n, ca, op, nfo))
        assert list(nfo) == Fp
        return outs

    def infer_contour(self, mel, contour):
        """infer() with the contour stage behind mel -> linear: 256 * (F' - 1) samples."""
        mel = np.ascontiguousarray(mel, dtype=np.float32)
        audio, n = _PF(), C.c_size_t()
        _check(lib.xdtts_griffinlim_infer_contour(self._h, _ptr(mel), mel.shape[0], mel.shape[1], C.byref(contour), C.byref(audio), C.byref(n)))
        return _take(audio, n.value, (n.value,))

    # -- pitch tracker and pitch targets: F0 per frame on the device, absolute-Hz targets and the pitch range ----
    def _f0_outs(self, Fs):
        n = len(Fs)
        raw, strength, f0 = ([np.empty(F, dtype=np.float32) for F in Fs] for _ in range(3))
        stats = (F0Stats * n)()
        return raw, strength, f0, stats

    def f0_linear_batch(self, S_list, opts=None):
        """The tracker alone on magnitudes S_u (n_bins, F_u), one k_f0_frames launch over all of them: (raw, strength, f0, stats),
        a list of one entry per utterance each -- raw F0 in Hz and the cepstral peak per frame, the smoothed F0 (0 = unvoiced),
        and an F0Stats."""
        Ss = [np.ascontiguousarray(S, dtype=np.float32) for S in S_list]
        n = len(Ss)
        raw, strength, f0, stats = self._f0_outs([S.shape[1] for S in Ss])
        sp = (C.c_void_p * n)(*[S.ctypes.data for S in Ss])
        nf = (C.c_size_t * n)(*[S.shape[1] for S in Ss])
        ptrs = [(C.c_void_p * n)(*[a.ctypes.data for a in arrs]) for arrs in (raw, strength, f0)]
        _check(lib.xdtts_griffinlim_f0_linear_batch(self._h, sp, nf, n, _opt_ref(opts), ptrs[0], ptrs[1], ptrs[2], stats))
        return raw, strength, f0, list(stats)

    def f0_linear(self, S, opts=None):
        """The tracker alone on one magnitude S (n_bins, F): (raw, strength, f0, stats)."""
        S = np.ascontiguousarray(S, dtype=np.float32)
        raw, strength, f0, stats = self._f0_outs([S.shape[1]])
        _check(lib.xdtts_griffinlim_f0_linear(self._h, _ptr(S), S.shape[1], _opt_ref(opts), _ptr(raw[0]), _ptr(strength[0]), _ptr(f0[0]), C.byref(stats[0])))
        return raw[0], strength[0], f0[0], stats[0]

    def f0(self, mel, opts=None):
        """The tracker on a mel (n_mels, F) through the handle's mel -> linear: (raw, strength, f0, stats)."""
        mel = np.ascontiguousarray(mel, dtype=np.float32)
        raw, strength, f0, stats = self._f0_outs([mel.shape[1]])
        _check(lib.xdtts_griffinlim_f0(self._h, _ptr(mel), mel.shape[0], mel.shape[1], _opt_ref(opts), _ptr(raw[0]), _ptr(strength[0]), _ptr(f0[0]), C.byref(stats[0])))
        return raw[0], strength[0], f0[0], stats[0]

    def f0_audio(self, audio, opts=None):
        """The tracker on audio at 22 050 Hz (the analysis entries' STFT magnitude, then the stage): (raw, strength, f0, stats),
        analysis_frames(len(audio)) entries each."""
        audio = np.ascontiguousarray(audio, dtype=np.float32)
        raw, strength, f0, stats = self._f0_outs([audio.size // 256 + 1])
        _check(lib.xdtts_griffinlim_f0_audio(self._h, _ptr(audio), audio.size, _opt_ref(opts), _ptr(raw[0]), _ptr(strength[0]), _ptr(f0[0]), C.byref(stats[0])))
        return raw[0], strength[0], f0[0], stats[0]

    def pitch_target_linear_batch(self, S_list, targets, contours=None, opts=None):
        """The application alone (parity hook): magnitudes S_u (n_bins, F_u), one PitchTarget each and contours that may be None
        -> (list of S'_u (n_bins, F'_u), list of ratio_u (F_u), list of F0Stats)."""
        Ss = [np.ascontiguousarray(S, dtype=np.float32) for S in S_list]
        n = len(Ss)
        ta, ca, keep = _target_arrays(targets, contours, n)
        Fp = [S.shape[1] if (keep is None or keep[u] is None) else prosody_contour_frames(keep[u], S.shape[1]) for u, S in enumerate(Ss)]
        outs = [np.empty((self.n_bins, max(f, 1)), dtype=np.float32) for f in Fp]
        ratios = [np.empty(S.shape[1], dtype=np.float32) for S in Ss]
        stats = (F0Stats * n)()
        sp = (C.c_void_p * n)(*[S.ctypes.data for S in Ss])
        op = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        rp = (C.c_void_p * n)(*[r.ctypes.data for r in ratios])
        nf = (C.c_size_t * n)(*[S.shape[1] for S in Ss])
        _check(lib.xdtts_griffinlim_pitch_target_linear_batch(self._h, sp, nf, n, _opt_ref(opts), ta, ca, op, rp, stats))
        return outs, ratios, list(stats)

    def pitch_target_linear(self, S, target, contour=None, opts=None):
        """The application alone on one magnitude: (S' (n_bins, F'), ratio (F), stats)."""
        S = np.ascontiguousarray(S, dtype=np.float32)
        Fp = S.shape[1] if contour is None else prosody_contour_frames(contour, S.shape[1])
        out = np.empty((self.n_bins, max(Fp, 1)), dtype=np.float32)
        ratio = np.empty(S.shape[1], dtype=np.float32)
        stats = F0Stats()
        _check(lib.xdtts_griffinlim_pitch_target_linear(self._h, _ptr(S), S.shape[1], _opt_ref(opts), C.byref(target), _opt_ref(contour), _ptr(out), _ptr(ratio), C.byref(stats)))
        return out, ratio, stats

    def infer_pitch_target(self, mel, target, contour=None, opts=None):
        """infer() with the tracker, the target and the contour stage behind mel -> linear; last_f0() then holds the stats."""
        mel = np.ascontiguousarray(mel, dtype=np.float32)
        audio, n = _PF(), C.c_size_t()
        _check(lib.xdtts_griffinlim_infer_pitch_target(self._h, _ptr(mel), mel.shape[0], mel.shape[1], _opt_ref(opts), C.byref(target), _opt_ref(contour), C.byref(audio), C.byref(n)))
        return _take(audio, n.value, (n.value,))

    def infer_batch_pitch_target(self, mels, targets, contours=None, opts=None):
        """infer_batch() with one PitchTarget per utterance (and contours that may be None)."""
        ms = [np.ascontiguousarray(m, dtype=np.float32) for m in mels]
        n = len(ms)
        ta, ca, keep = _target_arrays(targets, contours, n)
        ptrs = (C.c_void_p * n)(*[m.ctypes.data for m in ms])
        nf = (C.c_size_t * n)(*[m.shape[1] for m in ms])
        audios, ns = (_PF * n)(), (C.c_size_t * n)()
        _check(lib.xdtts_griffinlim_infer_batch_pitch_target(self._h, ptrs, ms[0].shape[0], nf, n, _opt_ref(opts), ta, ca, audios, ns))
        return [_take(audios[u], ns[u], (ns[u],)) for u in range(n)]

    def last_f0(self):
        """The F0Stats of each utterance of the last call that ran the tracker, in the caller's order ([] after a delivering call
        that ran none)."""
        n = C.c_size_t()
        _check(lib.xdtts_griffinlim_last_f0(self._h, None, 0, C.byref(n)))
        if n.value == 0:
            return []
        out = (F0Stats * n.value)()
        _check(lib.xdtts_griffinlim_last_f0(self._h, out, n.value, C.byref(n)))
        return list(out)

    # -- initial phase: the seeded random stream (0) or Single Pass Spectrogram Inversion (1) ----
    def set_phase_init(self, mode):
        """0: the seeded random stream (default), 1: SPSI on the magnitude that enters the loop; honoured by every entry
        that draws the initial phase itself (not by step, nor by infer_linear with a phase0)."""
        _check(lib.xdtts_griffinlim_set_phase_init(self._h, int(mode)))

    def get_phase_init(self):
        mode = C.c_int32()
        _check(lib.xdtts_griffinlim_get_phase_init(self._h, C.byref(mode)))
        return mode.value

    def spsi_phase(self, S):
        """The SPSI stage alone (parity hook), whatever the mode: S (n_bins, F) -> (turns (n_bins, F) uint32 in units of
        2^-32 turn, angles (n_bins, F, 2) (cos, sin): what infer_linear takes as phase0)."""
        turns, angles = self.spsi_phase_batch([S])
        return turns[0], angles[0]

    def spsi_phase_batch(self, S_list):
        """The ragged stage alone (parity hook): a list of S_u (n_bins, F_u) -> (list of turns, list of angles), every one
        the single hook's bit for bit."""
        Ss = [np.ascontiguousarray(S, dtype=np.float32) for S in S_list]
        n = len(Ss)
        turns = [np.empty(S.shape, dtype=np.uint32) for S in Ss]
        angles = [np.empty(S.shape + (2,), dtype=np.float32) for S in Ss]
        sp = (C.c_void_p * n)(*[S.ctypes.data for S in Ss])
        nf = (C.c_size_t * n)(*[S.shape[1] for S in Ss])
        tp = (C.c_void_p * n)(*[t.ctypes.data for t in turns])
        ap = (C.c_void_p * n)(*[a.ctypes.data for a in angles])
        if n == 1:
            _check(lib.xdtts_griffinlim_spsi_phase(self._h, sp[0], nf[0], tp[0], ap[0]))
        else:
            _check(lib.xdtts_griffinlim_spsi_phase_batch(self._h, sp, nf, n, tp, ap))
        return turns, angles

    # -- output rate: 22 050 Hz -> 8 .. 96 kHz behind the loop, in front of the output normalisation ----
    def set_output_rate(self, rate):
        """The rate of every delivered utterance (infer, infer_batch, synthesize* and their prosody / contour forms): 22050
        (default, nothing runs) or a supported rate (resample_plan): a polyphase windowed-sinc stage on the device.  Not honoured
        by infer_linear, step and the analysis entries."""
        _check(lib.xdtts_griffinlim_set_output_rate(self._h, int(rate)))

    def get_output_rate(self):
        rate = C.c_int32()
        _check(lib.xdtts_griffinlim_get_output_rate(self._h, C.byref(rate)))
        return rate.value

    def resample(self, audio, rate_out):
        """The stage alone (parity hook), whatever the handle's rate: audio at 22 050 Hz -> resample_plan(rate_out, len)["n_out"] samples."""
        return self.resample_batch([audio], rate_out)[0]

    def resample_batch(self, audios, rate_out):
        """The ragged stage alone (parity hook): one launch for all audios, every result the single hook's bit for bit."""
        xs = [np.ascontiguousarray(a, dtype=np.float32).ravel() for a in audios]
        n = len(xs)
        outs = [np.empty(max(resample_plan(rate_out, x.size)["n_out"], 1), dtype=np.float32) for x in xs]
        ip = (C.c_void_p * n)(*[x.ctypes.data for x in xs])
        op = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        ns = (C.c_size_t * n)(*[x.size for x in xs])
        no = (C.c_size_t * n)()
        if n == 1:
            _check(lib.xdtts_griffinlim_resample(self._h, ip[0], ns[0], int(rate_out), op[0], no))
        else:
            _check(lib.xdtts_griffinlim_resample_batch(self._h, ip, ns, n, int(rate_out), op, no))
        return [o[: no[u]] for u, o in enumerate(outs)]

    # -- loudness: BS.1770 integrated loudness under a true-peak ceiling, behind the resampler ----
    def set_loudness(self, target_lufs=None, ceiling_dbtp=None):
        """The level rule of every delivered utterance: a target in LUFS ([-70, 0]; None / NaN = off, the default) under a
        true-peak ceiling in dBTP ([-20, 6]; None / NaN = none).  When on it takes output_normalise's place, at the delivered
        rate; last_loudness() then has the measurement and the gain of each utterance."""
        t = float("nan") if target_lufs is None else float(target_lufs)
        c = float("nan") if ceiling_dbtp is None else float(ceiling_dbtp)
        _check(lib.xdtts_griffinlim_set_loudness(self._h, t, c))

    def get_loudness(self):
        t, c = C.c_float(), C.c_float()
        _check(lib.xdtts_griffinlim_get_loudness(self._h, C.byref(t), C.byref(c)))
        return t.value, c.value

    def last_loudness(self):
        """[Loudness] of the last delivering call, in the caller's order; [] without a target."""
        n = C.c_size_t()
        _check(lib.xdtts_griffinlim_last_loudness(self._h, None, 0, C.byref(n)))
        out = (Loudness * max(n.value, 1))()
        _check(lib.xdtts_griffinlim_last_loudness(self._h, out, n.value, C.byref(n)))
        return [out[i] for i in range(n.value)]

    def loudness(self, audio, rate):
        """The measurement alone on `audio` at `rate` (8000 .. 96000), whatever the handle's setting: a Loudness with gain 1."""
        return self.loudness_batch([audio], rate)[0]

    def loudness_batch(self, audios, rate):
        """The ragged measurement: one set of launches for all audios, every struct the single call's bit for bit."""
        xs = [np.ascontiguousarray(a, dtype=np.float32).ravel() for a in audios]
        n = len(xs)
        out = (Loudness * max(n, 1))()
        ip = (C.c_void_p * max(n, 1))(*[x.ctypes.data for x in xs])
        ns = (C.c_size_t * max(n, 1))(*[x.size for x in xs])
        if n == 1:
            _check(lib.xdtts_griffinlim_loudness(self._h, ip[0], ns[0], int(rate), out))
        else:
            _check(lib.xdtts_griffinlim_loudness_batch(self._h, ip, ns, n, int(rate), out))
        return [out[i] for i in range(n)]

    # -- timbre: vocal-tract length and breathiness, the voice of this handle ----
    def set_timbre(self, timbre=None):
        """The handle's voice from now on: a Timbre, or None for the default (the identity: nothing is launched).  Honoured by
        every entry that runs mel -> linear itself (infer*, synthesize*); infer_linear and the *_linear hooks do not."""
        _check(lib.xdtts_griffinlim_set_timbre(self._h, _opt_ref(timbre)))

    def get_timbre(self):
        t = Timbre()
        _check(lib.xdtts_griffinlim_get_timbre(self._h, C.byref(t)))
        return t

    def timbre_linear(self, S, timbre):
        """The timbre stage alone (parity hook), whatever the handle's setting: S (n_bins, F) -> S' (n_bins, F)."""
        S = np.ascontiguousarray(S, dtype=np.float32)
        out = np.empty_like(S)
        _check(lib.xdtts_griffinlim_timbre_linear(self._h, _ptr(S), S.shape[1], C.byref(timbre), _ptr(out)))
        return out

    def timbre_linear_batch(self, S_list, timbre_list):
        """The ragged stage alone (parity hook): a list of S_u (n_bins, F_u) and one Timbre each -> the list of S'_u, one
        k_timbre launch for all of them."""
        Ss = [np.ascontiguousarray(S, dtype=np.float32) for S in S_list]
        n = len(Ss)
        ts = list(timbre_list)
        if len(ts) != n:
            raise ValueError("timbre_linear_batch takes one Timbre per utterance: %d for %d utterances" % (len(ts), n))
        ta = (Timbre * max(n, 1))()
        for u, t in enumerate(ts):
            ta[u].vtl, ta[u].breath, ta[u].seed, ta[u].lifter, ta[u].log_floor = t.vtl, t.breath, t.seed, t.lifter, t.log_floor
        outs = [np.empty_like(S) for S in Ss]
        sp = (C.c_void_p * max(n, 1))(*[S.ctypes.data for S in Ss])
        op = (C.c_void_p * max(n, 1))(*[o.ctypes.data for o in outs])
        nf = (C.c_size_t * max(n, 1))(*[S.shape[1] for S in Ss])
        _check(lib.xdtts_griffinlim_timbre_linear_batch(self._h, sp, nf, n, ta, op))
        return outs

    # -- clean-up: spectral subtraction with a floor and a tone curve, the first stage behind mel -> linear ----
    def set_denoise(self, denoise=None, profile=None):
        """The handle's clean-up stage from now on: a Denoise, or None for off (the default: nothing is launched), with an
        optional noise profile (n_bins floats, e.g. noise_profile() of a silent utterance of the checkpoint).  Honoured by every
        entry that runs mel -> linear itself (infer*, synthesize*); infer_linear and the *_linear hooks do not."""
        p = None if profile is None else np.ascontiguousarray(profile, dtype=np.float32).ravel()
        if p is not None and p.size != self.n_bins:
            raise ValueError("a noise profile has %d bins, got %d" % (self.n_bins, p.size))
        _check(lib.xdtts_griffinlim_set_denoise(self._h, _opt_ref(denoise), None if p is None else _ptr(p)))

    def get_denoise(self):
        """(Denoise, profile or None) as set."""
        d, flag = Denoise(), C.c_int32()
        p = np.zeros(self.n_bins, dtype=np.float32)
        _check(lib.xdtts_griffinlim_get_denoise(self._h, C.byref(d), _ptr(p), C.byref(flag)))
        return d, (p if flag.value else None)

    def last_denoise(self):
        """The DenoiseStats of each utterance of the last call that ran the stage, in the caller's order ([] after a delivering
        call with the setting off)."""
        n = C.c_size_t()
        _check(lib.xdtts_griffinlim_last_denoise(self._h, None, 0, C.byref(n)))
        if n.value == 0:
            return []
        out = (DenoiseStats * n.value)()
        _check(lib.xdtts_griffinlim_last_denoise(self._h, out, n.value, C.byref(n)))
        return list(out)

    def denoise_linear(self, S, denoise, profile=None):
        """The clean-up stage alone (parity hook), whatever the handle's setting: S (n_bins, F) -> S' (n_bins, F)."""
        S = np.ascontiguousarray(S, dtype=np.float32)
        out = np.empty_like(S)
        p = None if profile is None else np.ascontiguousarray(profile, dtype=np.float32).ravel()
        _check(lib.xdtts_griffinlim_denoise_linear(self._h, _ptr(S), S.shape[1], C.byref(denoise), None if p is None else _ptr(p), _ptr(out)))
        return out

    def denoise_linear_batch(self, S_list, denoise_list, profile=None):
        """The ragged stage alone (parity hook): a list of S_u (n_bins, F_u), one Denoise each and one shared profile or None
        -> the list of S'_u, every one the single hook's bit for bit."""
        Ss = [np.ascontiguousarray(S, dtype=np.float32) for S in S_list]
        n = len(Ss)
        ds = list(denoise_list)
        if len(ds) != n:
            raise ValueError("denoise_linear_batch takes one Denoise per utterance: %d for %d utterances" % (len(ds), n))
        da = (Denoise * max(n, 1))()
        for u, d in enumerate(ds):
            C.memmove(C.byref(da[u]), C.byref(d), C.sizeof(Denoise))
        outs = [np.empty_like(S) for S in Ss]
        sp = (C.c_void_p * max(n, 1))(*[S.ctypes.data for S in Ss])
        op = (C.c_void_p * max(n, 1))(*[o.ctypes.data for o in outs])
        nf = (C.c_size_t * max(n, 1))(*[S.shape[1] for S in Ss])
        p = None if profile is None else np.ascontiguousarray(profile, dtype=np.float32).ravel()
        _check(lib.xdtts_griffinlim_denoise_linear_batch(self._h, sp, nf, n, da, None if p is None else _ptr(p), op))
        return outs

    def noise_profile(self, S, quantile=0.5):
        """The selection alone: per bin the order statistic `quantile` over the frames of S (n_bins, F) -> (n_bins,)."""
        S = np.ascontiguousarray(S, dtype=np.float32)
        out = np.empty(S.shape[0], dtype=np.float32)
        _check(lib.xdtts_griffinlim_noise_profile(self._h, _ptr(S), S.shape[1], float(quantile), _ptr(out)))
        return out

    # -- limiter: look-ahead true-peak limiter where the loudness stage scaled ----
    def set_limiter(self, lookahead_us=0):
        """With a target and a ceiling set (set_loudness): the gain is formed without the ceiling and a look-ahead limiter of
        `lookahead_us` microseconds (500 .. 10000; 0 / None = off, the default) keeps the ceiling around the peaks only.
        last_limiter() then has the stats of each utterance; last_loudness()[u].gain is the static gain."""
        _check(lib.xdtts_griffinlim_set_limiter(self._h, int(lookahead_us or 0)))

    def get_limiter(self):
        v = C.c_int32()
        _check(lib.xdtts_griffinlim_get_limiter(self._h, C.byref(v)))
        return v.value

    def last_limiter(self):
        """[LimiterStats] of the last delivering call, in the caller's order; [] unless a target, a ceiling and a limiter are set."""
        n = C.c_size_t()
        _check(lib.xdtts_griffinlim_last_limiter(self._h, None, 0, C.byref(n)))
        out = (LimiterStats * max(n.value, 1))()
        _check(lib.xdtts_griffinlim_last_limiter(self._h, out, n.value, C.byref(n)))
        return [out[i] for i in range(n.value)]

    def limit(self, audio, rate, gain0, ceiling_lin, lookahead_us):
        """The stage alone on `audio`, whatever the handle's settings: (out, LimiterStats), the bits of limiter_reference()."""
        outs, stats = self.limit_batch([audio], rate, gain0, ceiling_lin, lookahead_us)
        return outs[0], stats[0]

    def limit_batch(self, audios, rate, gain0, ceiling_lin, lookahead_us):
        """The ragged stage: one set of launches for all audios, every output and struct the single call's bit for bit."""
        xs = [np.ascontiguousarray(a, dtype=np.float32).ravel() for a in audios]
        n = len(xs)
        outs = [np.empty(x.size, dtype=np.float32) for x in xs]
        stats = (LimiterStats * max(n, 1))()
        ip = (C.c_void_p * max(n, 1))(*[x.ctypes.data for x in xs])
        op = (C.c_void_p * max(n, 1))(*[o.ctypes.data for o in outs])
        ns = (C.c_size_t * max(n, 1))(*[x.size for x in xs])
        if n == 1:
            _check(lib.xdtts_griffinlim_limit(self._h, ip[0], ns[0], int(rate), float(gain0), float(ceiling_lin), int(lookahead_us),
                                              op[0], stats))
        else:
            _check(lib.xdtts_griffinlim_limit_batch(self._h, ip, ns, n, int(rate), float(gain0), float(ceiling_lin),
                                                    int(lookahead_us), op, stats))
        return outs, [stats[i] for i in range(n)]

    # -- compressor: tent-envelope dynamic range compressor in front of the level stage ----
    def set_compressor(self, compressor=None):
        """The handle's compressor from now on: a Compressor, or None for off (the default).  It runs behind the output rate and
        in front of the output normalisation / loudness target / limiter, on every entry that delivers an utterance;
        last_compressor() then has the stats of each utterance.  The identity (ratio 1, makeup 0) launches nothing."""
        _check(lib.xdtts_griffinlim_set_compressor(self._h, _opt_ref(compressor)))

    def get_compressor(self):
        """The Compressor that is set, or None where the stage is off."""
        c, on = Compressor(), C.c_int32()
        _check(lib.xdtts_griffinlim_get_compressor(self._h, C.byref(c), C.byref(on)))
        return c if on.value else None

    def last_compressor(self):
        """[CompressorStats] of the last delivering call, in the caller's order; [] unless a compressor other than the identity is set."""
        n = C.c_size_t()
        _check(lib.xdtts_griffinlim_last_compressor(self._h, None, 0, C.byref(n)))
        out = (CompressorStats * max(n.value, 1))()
        _check(lib.xdtts_griffinlim_last_compressor(self._h, out, n.value, C.byref(n)))
        return [out[i] for i in range(n.value)]

    def compress(self, audio, rate, compressor):
        """The stage alone on `audio`, whatever the handle's settings: (out, CompressorStats), the bits of compressor_reference()."""
        outs, stats = self.compress_batch([audio], rate, compressor)
        return outs[0], stats[0]

    def compress_batch(self, audios, rate, compressor):
        """The ragged stage: one set of launches for all audios, every output and struct the single call's bit for bit."""
        xs = [np.ascontiguousarray(a, dtype=np.float32).ravel() for a in audios]
        n = len(xs)
        outs = [np.empty(x.size, dtype=np.float32) for x in xs]
        stats = (CompressorStats * max(n, 1))()
        ip = (C.c_void_p * max(n, 1))(*[x.ctypes.data for x in xs])
        op = (C.c_void_p * max(n, 1))(*[o.ctypes.data for o in outs])
        ns = (C.c_size_t * max(n, 1))(*[x.size for x in xs])
        if n == 1:
            _check(lib.xdtts_griffinlim_compress(self._h, ip[0], ns[0], int(rate), C.byref(compressor), op[0], stats))
        else:
            _check(lib.xdtts_griffinlim_compress_batch(self._h, ip, ns, n, int(rate), C.byref(compressor), op, stats))
        return outs, [stats[i] for i in range(n)]

    # -- silence: edge silence trimmed, pauses capped; the last stage of the delivery chain ----
    def set_silence(self, silence=None):
        """The handle's silence stage from now on: a Silence, or None for off (the default).  It runs behind the level stage on
        every entry that delivers an utterance, which then returns n_out samples; last_silence() has the stats of each."""
        _check(lib.xdtts_griffinlim_set_silence(self._h, _opt_ref(silence)))

    def get_silence(self):
        """The Silence that is set, or None where the stage is off."""
        s, on = Silence(), C.c_int32()
        _check(lib.xdtts_griffinlim_get_silence(self._h, C.byref(s), C.byref(on)))
        return s if on.value else None

    def last_silence(self):
        """[SilenceStats] of the last delivering call, in the caller's order; [] unless the stage is set."""
        n = C.c_size_t()
        _check(lib.xdtts_griffinlim_last_silence(self._h, None, 0, C.byref(n)))
        out = (SilenceStats * max(n.value, 1))()
        _check(lib.xdtts_griffinlim_last_silence(self._h, out, n.value, C.byref(n)))
        return [out[i] for i in range(n.value)]

    def trim(self, audio, rate, silence):
        """The stage alone on `audio`, whatever the handle's settings: (out[:n_out], SilenceStats), the bits of silence_reference()."""
        outs, stats = self.trim_batch([audio], rate, silence)
        return outs[0], stats[0]

    def trim_batch(self, audios, rate, silence):
        """The ragged stage: one set of launches for all audios, every output and struct the single call's bit for bit."""
        xs = [np.ascontiguousarray(a, dtype=np.float32).ravel() for a in audios]
        n = len(xs)
        outs = [np.empty(x.size, dtype=np.float32) for x in xs]
        stats = (SilenceStats * max(n, 1))()
        ip = (C.c_void_p * max(n, 1))(*[x.ctypes.data for x in xs])
        op = (C.c_void_p * max(n, 1))(*[o.ctypes.data for o in outs])
        ns = (C.c_size_t * max(n, 1))(*[x.size for x in xs])
        if n == 1:
            _check(lib.xdtts_griffinlim_trim(self._h, ip[0], ns[0], int(rate), C.byref(silence), op[0], stats))
        else:
            _check(lib.xdtts_griffinlim_trim_batch(self._h, ip, ns, n, int(rate), C.byref(silence), op, stats))
        return [o[:stats[i].n_out] for i, o in enumerate(outs)], [stats[i] for i in range(n)]

    # -- stream: a sequence joined with its gaps, faded, levelled and encoded on the device ----
    def join(self, audios, gaps=None, rate=SAMPLE_RATE, opts=None, guard=0):
        """xdtts_griffinlim_join: the stage alone on the caller's audios (fp32, each read where it lies: a view's address decides
        the kernel's load route).  gaps = n + 1 lengths in samples, or None.  Returns (stream, offsets): stream is float32 /
        int16 / uint8 by opts.format.  guard= extra bytes behind the stream, filled with 0xA5 and returned with it (the tests'
        guard band)."""
        xs = [np.ascontiguousarray(a, dtype=np.float32).ravel() for a in audios]
        n = len(xs)
        o = opts if opts is not None else StreamOpts()
        ns = (C.c_size_t * max(n, 1))(*[x.size for x in xs])
        ip = (C.c_void_p * max(n, 1))(*[(x.ctypes.data if x.size else None) for x in xs])
        gp = None if gaps is None else (C.c_size_t * (n + 1))(*[int(v) for v in gaps])
        offs, tot = (C.c_size_t * max(n, 1))(), C.c_size_t()
        _check(lib.xdtts_stream_plan(ns, n, gp, offs, C.byref(tot)))
        sb = int(lib.xdtts_stream_sample_bytes(o.format))
        raw = np.full(tot.value * sb + int(guard), 0xA5, dtype=np.uint8)
        _check(lib.xdtts_griffinlim_join(self._h, ip, ns, n, gp, int(rate), C.byref(o), _ptr(raw), tot.value * sb, offs, C.byref(tot)))
        out = raw[: tot.value * sb].view(_STREAM_DTYPE[o.format])
        offsets = [int(offs[u]) for u in range(n)]
        return (out, offsets, raw[tot.value * sb:]) if guard else (out, offsets)

    # -- analysis: audio -> magnitude -> mel under the handle's conventions, spectral convergence ----
    def analysis_frames(self, n_samples):
        return int(lib.xdtts_griffinlim_analysis_frames(self._h, int(n_samples)))

    def analyze(self, audio, mel_floor=1e-5, want_S=True, want_mel=True):
        """librosa.stft(audio, 1024, hop 256) -> |.| -> mel basis -> compression, the inverse of infer's conventions (power,
        power_mode, mel_decompress).  Returns (S (n_bins, F), mel (n_mels, F)), F = len(audio) // 256 + 1; None where not wanted."""
        S, mel = self.analyze_batch([audio], mel_floor, want_S, want_mel)
        return (S[0] if want_S else None), (mel[0] if want_mel else None)

    def analyze_batch(self, audios, mel_floor=1e-5, want_S=True, want_mel=True):
        """analyze() for a list of audios in one call (one magnitude launch, one projection); every result is the single
        call's bit for bit.  Returns (list of S or None, list of mel or None)."""
        ys = [np.ascontiguousarray(a, dtype=np.float32).ravel() for a in audios]
        n = len(ys)
        Fs = [self.analysis_frames(max(y.size, 1)) for y in ys]
        S = [np.empty((self.n_bins, F), dtype=np.float32) for F in Fs] if want_S else None
        mel = [np.empty((self.n_mels, F), dtype=np.float32) for F in Fs] if want_mel else None
        ptrs = (C.c_void_p * n)(*[y.ctypes.data for y in ys])
        ns = (C.c_size_t * n)(*[y.size for y in ys])
        Sp = (C.c_void_p * n)(*[a.ctypes.data for a in S]) if want_S else None
        Mp = (C.c_void_p * n)(*[a.ctypes.data for a in mel]) if want_mel else None
        nf = (C.c_size_t * n)()
        _check(lib.xdtts_griffinlim_analyze_batch(self._h, ptrs, ns, n, mel_floor, Sp, Mp, nf))
        assert list(nf) == Fs
        return S, mel

    def spectral_convergence(self, audio, S, fit_gain=False):
        """(|| a |STFT(audio)| - S || / || S ||, a) against the target magnitude S (n_bins, F); a = 1, or with fit_gain the
        least-squares gain (for audio that went through output_normalise)."""
        y = np.ascontiguousarray(audio, dtype=np.float32).ravel()
        S = np.ascontiguousarray(S, dtype=np.float32)
        out = (C.c_float * 2)()
        _check(lib.xdtts_griffinlim_spectral_convergence(self._h, _ptr(y), y.size, _ptr(S), S.shape[1], 1 if fit_gain else 0, C.byref(out)))
        return float(out[0]), float(out[1])

    def analysis_timings(self):
        ms = (C.c_float * 3)()
        _check(lib.xdtts_griffinlim_analysis_timings(self._h, C.byref(ms)))
        return {"magnitude_ms": ms[0], "projection_ms": ms[1], "total_ms": ms[2]}


def create_griffin_lim(device_id=0, iters=30, seed=0):
    """create_griffin_lim() -- src/tacotron2/mod.rs:441-458 (sr 22050, n_fft 1024, 80 mels, fmin 0,
    fmax 8000, noverlap 768, power 1.7, 30 iterations, momentum 0.99)."""
    mel_basis = create_mel_filter_bank(22050.0, 1024, 80, 0.0, 8000.0)
    return GriffinLim(mel_basis, 1024 - 256, 1.7, iters, 0.99, device_id=device_id, seed=seed)


def prosody_frames(n_frames, rate):
    """xdtts_prosody_frames: the frame count behind the prosody stage (host arithmetic); 0 for a bad argument."""
    return int(lib.xdtts_prosody_frames(int(n_frames), float(rate)))


def prosody_contour_frames(contour, n_frames):
    """xdtts_prosody_contour_frames: the frame count behind the contour stage (host arithmetic); 0 for a bad argument."""
    return int(lib.xdtts_prosody_contour_frames(C.byref(contour), int(n_frames)))


def f0_plan(opts=None):
    """xdtts_f0_plan: (q_lo, q_hi), the quefrency range of the options (host arithmetic); raises on a bad field."""
    lo, hi = C.c_int32(), C.c_int32()
    _check(lib.xdtts_f0_plan(_opt_ref(opts), C.byref(lo), C.byref(hi)))
    return lo.value, hi.value


def f0_track_reference(raw, strength, opts=None, target=None):
    """xdtts_f0_track_reference: the utterance stage on the host from raw / strength arrays -> (f0, ratio, F0Stats)."""
    raw = np.ascontiguousarray(raw, dtype=np.float32)
    strength = np.ascontiguousarray(strength, dtype=np.float32)
    if raw.shape != strength.shape or raw.ndim != 1:
        raise ValueError("raw and strength are two vectors of one length")
    f0, ratio, stats = np.empty(raw.size, dtype=np.float32), np.empty(raw.size, dtype=np.float32), F0Stats()
    _check(lib.xdtts_f0_track_reference(_ptr(raw), _ptr(strength), raw.size, _opt_ref(opts), _opt_ref(target), _ptr(f0), _ptr(ratio), C.byref(stats)))
    return f0, ratio, stats


def prosody_contour_table(contour, n_frames):
    """xdtts_prosody_contour_table: (c uint32, pitch float32, gain float32), n_frames entries each -- the table the device reads."""
    n = int(n_frames)
    c, pitch, gain = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.float32)
    _check(lib.xdtts_prosody_contour_table(C.byref(contour), n, _ptr(c), _ptr(pitch), _ptr(gain)))
    return c[:n], pitch[:n], gain[:n]


def resample_plan(rate_out, n_in=0):
    """xdtts_resample_plan (host arithmetic): {"L", "M", "half_len", "n_out"} of the output-rate stage for n_in samples at
    22 050 Hz; XdttsError (BAD_ARG) for an unsupported rate."""
    L, M, H, n = C.c_int32(), C.c_int32(), C.c_int32(), C.c_size_t()
    _check(lib.xdtts_resample_plan(int(rate_out), int(n_in), C.byref(L), C.byref(M), C.byref(H), C.byref(n)))
    return {"L": L.value, "M": M.value, "half_len": H.value, "n_out": n.value}


def resample_filter(rate_out):
    """xdtts_resample_filter: the library's own fp32 taps h[-H .. H] of the output-rate stage (host arithmetic)."""
    n = C.c_size_t()
    _check(lib.xdtts_resample_filter(int(rate_out), None, 0, C.byref(n)))
    taps = np.empty(n.value, dtype=np.float32)
    _check(lib.xdtts_resample_filter(int(rate_out), _ptr(taps), taps.size, C.byref(n)))
    return taps


def loudness_plan(rate, n=0):
    """xdtts_loudness_plan (host arithmetic): {"hop", "n_blocks"} of the loudness stage for n samples at `rate`."""
    h, nb = C.c_int32(), C.c_size_t()
    _check(lib.xdtts_loudness_plan(int(rate), int(n), C.byref(h), C.byref(nb)))
    return {"hop": h.value, "n_blocks": nb.value}


def loudness_filter(rate):
    """xdtts_loudness_filter: the K-weighting at `rate` as ((b_shelf, a_shelf), (b_highpass, a_highpass)), fp64, a0 = 1."""
    c = np.zeros(10, dtype=np.float64)
    _check(lib.xdtts_loudness_filter(int(rate), _ptr(c)))
    one = np.ones(1)
    return (c[0:3].copy(), np.concatenate([one, c[3:5]])), (c[5:8].copy(), np.concatenate([one, c[8:10]]))


def true_peak_filter():
    """xdtts_true_peak_filter: the library's own fp32 taps, [3][24]: taps[p - 1][j + 12] = t[4 j + p]."""
    t = np.zeros((3, 24), dtype=np.float32)
    _check(lib.xdtts_true_peak_filter(_ptr(t)))
    return t


def limiter_plan(rate, lookahead_us):
    """xdtts_limiter_plan (host arithmetic): {"half_width", "tile"} of the limiter at `rate` with `lookahead_us` microseconds."""
    h, t = C.c_int32(), C.c_int32()
    _check(lib.xdtts_limiter_plan(int(rate), int(lookahead_us), C.byref(h), C.byref(t)))
    return {"half_width": h.value, "tile": t.value}


def limiter_window(rate, lookahead_us):
    """xdtts_limiter_window: the library's own fp32 smoothing weights w[-H .. H]."""
    w = np.zeros(2 * limiter_plan(rate, lookahead_us)["half_width"] + 1, dtype=np.float32)
    _check(lib.xdtts_limiter_window(int(rate), int(lookahead_us), _ptr(w)))
    return w


def limiter_reference(audio, rate, gain0, ceiling_lin, lookahead_us):
    """xdtts_limiter_reference: the definition sample by sample in plain C++ on the host: (out, LimiterStats)."""
    x = np.ascontiguousarray(audio, dtype=np.float32).ravel()
    out = np.empty(x.size, dtype=np.float32)
    st = LimiterStats()
    _check(lib.xdtts_limiter_reference(_ptr(x) if x.size else None, x.size, int(rate), float(gain0), float(ceiling_lin), int(lookahead_us),
                                       _ptr(out) if x.size else None, C.byref(st)))
    return out, st


def compressor_preset(which):
    """xdtts_compressor_preset: 0 the default (the identity), 1 "drc" (-24 dB, 3:1, knee 6 dB, 5 ms / 100 ms, no make-up)."""
    c = Compressor()
    _check(lib.xdtts_compressor_preset(int(which), C.byref(c)))
    return c


def compressor_plan(rate, compressor):
    """xdtts_compressor_plan (host arithmetic): {"alpha", "rho", "T", "W", "tile"} -- slopes per sample, threshold and knee, all in
    2^-16 octaves, and the samples per workgroup."""
    v = [C.c_int32() for _ in range(5)]
    _check(lib.xdtts_compressor_plan(int(rate), C.byref(compressor), *[C.byref(x) for x in v]))
    return dict(zip(("alpha", "rho", "T", "W", "tile"), (x.value for x in v)))


def compressor_level(audio):
    """xdtts_compressor_level: the library's own lvl(|audio|), int32 in 2^-16 octaves (host arithmetic)."""
    x = np.ascontiguousarray(audio, dtype=np.float32).ravel()
    l = np.zeros(x.size, dtype=np.int32)
    _check(lib.xdtts_compressor_level(_ptr(x) if x.size else None, x.size, _ptr(l) if x.size else None))
    return l


def compressor_envelope(audio, rate, compressor):
    """xdtts_compressor_envelope: the integer envelope V of the definition (host arithmetic, the serial form)."""
    x = np.ascontiguousarray(audio, dtype=np.float32).ravel()
    V = np.zeros(x.size, dtype=np.int32)
    _check(lib.xdtts_compressor_envelope(_ptr(x) if x.size else None, x.size, int(rate), C.byref(compressor), _ptr(V) if x.size else None))
    return V


def compressor_reference(audio, rate, compressor):
    """xdtts_compressor_reference: the definition sample by sample in plain C++ on the host: (out, CompressorStats)."""
    x = np.ascontiguousarray(audio, dtype=np.float32).ravel()
    out = np.empty(x.size, dtype=np.float32)
    st = CompressorStats()
    _check(lib.xdtts_compressor_reference(_ptr(x) if x.size else None, x.size, int(rate), C.byref(compressor), _ptr(out) if x.size else None,
                                          C.byref(st)))
    return out, st


def silence_plan(rate, silence):
    """xdtts_silence_plan (host arithmetic): {"W", "min_w", "lead_w", "trail_w", "pause_w", "fade", "tfac"} -- the window in
    samples, the settings in windows, the fade in samples, and the threshold's factor (a float32)."""
    v = [C.c_int32() for _ in range(6)]
    t = C.c_float()
    _check(lib.xdtts_silence_plan(int(rate), C.byref(silence), *[C.byref(x) for x in v], C.byref(t)))
    d = dict(zip(("W", "min_w", "lead_w", "trail_w", "pause_w", "fade"), (x.value for x in v)))
    d["tfac"] = np.float32(t.value)
    return d


def silence_keep(audio, rate, silence):
    """xdtts_silence_keep: the per-window decisions, uint8 [ceil(n / W)] (host arithmetic)."""
    x = np.ascontiguousarray(audio, dtype=np.float32).ravel()
    W = int(rate) // 200
    keep = np.zeros(max((x.size + W - 1) // max(W, 1), 1), dtype=np.uint8)
    _check(lib.xdtts_silence_keep(_ptr(x) if x.size else None, x.size, int(rate), C.byref(silence), _ptr(keep)))
    return keep


def silence_reference(audio, rate, silence):
    """xdtts_silence_reference: the definition as serial plain C++ on the host: (out[:n_out], SilenceStats)."""
    x = np.ascontiguousarray(audio, dtype=np.float32).ravel()
    out = np.empty(max(x.size, 1), dtype=np.float32)
    st = SilenceStats()
    _check(lib.xdtts_silence_reference(_ptr(x) if x.size else None, x.size, int(rate), C.byref(silence), _ptr(out), C.byref(st)))
    return out[:st.n_out].copy(), st


def denoise_rank(n_frames, quantile):
    """r = floor(quantile * (F - 1)) of the clean-up stage's selection.  Host arithmetic."""
    return int(lib.xdtts_denoise_rank(int(n_frames), float(quantile)))


def denoise_floor(floor_db):
    """gmin = (float) 10 ** (floor_db / 20) as the clean-up stage forms it.  Host arithmetic."""
    return np.float32(lib.xdtts_denoise_floor(float(floor_db)))


def denoise_tone(denoise):
    """E[513] of a Denoise's tone curve (all 1 without points).  Host arithmetic."""
    E = np.empty(513, dtype=np.float32)
    _check(lib.xdtts_denoise_tone(C.byref(denoise), _ptr(E)))
    return E


def denoise_reference(S, denoise, profile=None):
    """The clean-up stage's definition as serial plain C++ on the host: S (513, F) -> (S' (513, F), DenoiseStats)."""
    S = np.ascontiguousarray(S, dtype=np.float32)
    out = np.empty_like(S)
    st = DenoiseStats()
    p = None if profile is None else np.ascontiguousarray(profile, dtype=np.float32).ravel()
    if p is not None and p.size != 513:
        raise ValueError("a noise profile has 513 bins, got %d" % p.size)
    _check(lib.xdtts_denoise_reference(_ptr(S), S.shape[1], C.byref(denoise), None if p is None else _ptr(p), _ptr(out), C.byref(st)))
    return out, st


def timbre_noise_bits(seed, frame, bin):
    """n of the timbre stage's breath noise at cell (frame, bin): 23 bits, a function of (seed, frame, bin) alone.  Host arithmetic."""
    return int(lib.xdtts_timbre_noise_bits(int(seed) & 0xFFFFFFFF, int(frame), int(bin)))


def stream_sample_bytes(format):
    return int(lib.xdtts_stream_sample_bytes(int(format)))


def stream_plan(n, gaps=None):
    """xdtts_stream_plan (host arithmetic): (offsets, total) of utterances of n[u] samples joined with gaps[0 .. len(n)]."""
    U = len(n)
    ns = (C.c_size_t * max(U, 1))(*[int(v) for v in n])
    gp = None if gaps is None else (C.c_size_t * (U + 1))(*[int(v) for v in gaps])
    offs, tot = (C.c_size_t * max(U, 1))(), C.c_size_t()
    _check(lib.xdtts_stream_plan(ns, U, gp, offs, C.byref(tot)))
    return [int(offs[u]) for u in range(U)], int(tot.value)


def stream_fade_table(fade):
    """xdtts_stream_fade_table: T[j] = 0.5 - 0.5 cos(pi (j + 0.5) / fade) as the library's own fp32 values."""
    w = np.zeros(int(fade), dtype=np.float32)
    _check(lib.xdtts_stream_fade_table(int(fade), _ptr(w) if w.size else None))
    return w


def stream_encode_sample(x, format, dither=0, seed=0, k=0):
    """xdtts_stream_encode_sample: one sample behind fade and gain at stream position k -> its fp32 / int16 / uint8 value."""
    out = np.zeros(4, dtype=np.uint8)
    _check(lib.xdtts_stream_encode_sample(float(x), int(format), int(dither), int(seed), int(k), _ptr(out)))
    return out[: stream_sample_bytes(format)].view(_STREAM_DTYPE[int(format)])[0]


def synthesize_document(tacotron2, vocoder, ids_list, gaps=None, stream_opts=None, splits_list=None, opts=None, want_mels=True, prosody=None):
    """XdTts::generate_audio (src/lib.rs:60-108): the utterances run as synthesize_sequence runs them, their audio stays on the
    device and leaves as ONE stream -- joined with the gaps (n + 1 lengths in samples at the vocoder's output rate), faded,
    levelled and encoded as stream_opts says (xdtts_synthesize_document).  Returns (mels or None, stream, offsets)."""
    n = len(ids_list)
    idv = [np.ascontiguousarray(x, dtype=np.int64) for x in ids_list]
    spv = [None if (splits_list is None or splits_list[u] is None) else np.ascontiguousarray(splits_list[u], dtype=np.uintp) for u in range(n)]
    ids_p = (C.c_void_p * n)(*[x.ctypes.data for x in idv])
    n_ids = (C.c_size_t * n)(*[x.size for x in idv])
    sp_p = (C.c_void_p * n)(*[(None if s is None else s.ctypes.data) for s in spv])
    n_sp = (C.c_size_t * n)(*[(0 if s is None else s.size) for s in spv])
    o = stream_opts if stream_opts is not None else StreamOpts()
    gp = None if gaps is None else (C.c_size_t * (n + 1))(*[int(v) for v in gaps])
    mels = (_PF * n)() if want_mels else None
    nf, offs = (C.c_size_t * n)(), (C.c_size_t * n)()
    stream, tot = C.c_void_p(), C.c_size_t()
    _check(lib.xdtts_synthesize_document(tacotron2._h, vocoder._h, ids_p, n_ids, sp_p, n_sp, n, C.byref(opts) if opts else None,
                                         None if prosody is None else _prosody_array(prosody, n), gp, C.byref(o), mels, nf,
                                         C.byref(stream), offs, C.byref(tot)))
    nbytes = tot.value * stream_sample_bytes(o.format)
    words = _take(C.cast(stream, _PF), (nbytes + 3) // 4, ((nbytes + 3) // 4,))  # (the pool's buffer, released with the last view)
    out = words.view(np.uint8)[:nbytes].view(_STREAM_DTYPE[o.format])
    out_m = [_take(mels[u], N_MEL * nf[u], (N_MEL, nf[u])) for u in range(n)] if want_mels else None
    return out_m, out, [int(offs[u]) for u in range(n)]


def synthesize(tacotron2, vocoder, ids, splits=None, opts=None, prosody=None, contour=None, target=None, f0_opts=None, contour_at_ids=None):
    """XdTts::infer (src/lib.rs:110-159): mel-gen then vocoder, mel kept in HBM in between.  prosody= (a Prosody) changes rate
    and pitch in the vocoder (xdtts_synthesize_ids_prosody): the mel returned is Tacotron2's own, the audio the modified one.
    contour= (a ProsodyContour) does so with values that vary inside the utterance (xdtts_synthesize_ids_contour).  target= (a
    PitchTarget, with contour= or alone; f0_opts= an F0Opts) tracks the utterance's F0 on the device and moves its median to an
    absolute pitch and / or scales its range (xdtts_synthesize_ids_pitch_target); vocoder.last_f0() then holds the stats.
    contour_at_ids= (a ProsodyContour whose pos are positions in ids, 0 .. len(ids); alone) anchors the contour at ids through
    the durations of this decode (xdtts_synthesize_ids_contour_at_ids)."""
    _one_of(prosody, contour)
    if contour_at_ids is not None and (prosody is not None or contour is not None or target is not None):
        raise ValueError("contour_at_ids= goes alone")
    if target is not None and prosody is not None:
        raise ValueError("target= goes with contour=, not with prosody=")
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    sp = None if splits is None else np.ascontiguousarray(splits, dtype=np.uintp)
    mel, nf, audio, ns = _PF(), C.c_size_t(), _PF(), C.c_size_t()
    head = (tacotron2._h, vocoder._h, _ptr(ids), ids.size, None if sp is None else _ptr(sp), 0 if sp is None else sp.size, C.byref(opts) if opts else None)
    tail = (C.byref(mel), C.byref(nf), C.byref(audio), C.byref(ns))
    if contour_at_ids is not None:
        _check(lib.xdtts_synthesize_ids_contour_at_ids(*head, C.byref(contour_at_ids), *tail))
    elif target is not None:
        _check(lib.xdtts_synthesize_ids_pitch_target(*head, _opt_ref(f0_opts), C.byref(target), _opt_ref(contour), *tail))
    elif contour is not None:
        _check(lib.xdtts_synthesize_ids_contour(*head, C.byref(contour), *tail))
    elif prosody is None:
        _check(lib.xdtts_synthesize_ids(*head, *tail))
    else:
        _check(lib.xdtts_synthesize_ids_prosody(*head, C.byref(prosody), *tail))
    return _take(mel, N_MEL * nf.value, (N_MEL, nf.value)), _take(audio, ns.value, (ns.value,))


def synthesize_batch(tacotron2, vocoder, utterance_chunks, opts=None, fixed_steps=None, want_mels=True, prosody=None, contour=None,
                     target=None, f0_opts=None, contour_at_ids=None):
    """XdTts::infer (src/lib.rs:110-159) for several utterances in one call: `utterance_chunks[u]` is the
    list of <=window-id chunks of utterance u (find_splits + the trailing split, mod.rs:399,412-414);
    `fixed_steps`, if given, holds one frame count per chunk in the same nested shape.  All chunks decode
    in one lock-step batch and the vocoder batch reads the concatenated mel in HBM.  Returns
    (mels or None, audios), one entry per utterance.  prosody= (a list of one Prosody per utterance): the mels stay Tacotron2's
    own, the audios go through the rate / pitch stage (xdtts_synthesize_batch_prosody); contour= (a list of one ProsodyContour per
    utterance) likewise with the contour stage (xdtts_synthesize_batch_contour).  target= (a list of one PitchTarget per
    utterance; contour= may then hold None entries) runs the pitch tracker and the targets (xdtts_synthesize_batch_pitch_target).
    contour_at_ids= (a list of one ProsodyContour per utterance, pos in ids of that utterance; alone):
    xdtts_synthesize_batch_contour_at_ids."""
    _one_of(prosody, contour)
    if contour_at_ids is not None and (prosody is not None or contour is not None or target is not None):
        raise ValueError("contour_at_ids= goes alone")
    if target is not None and prosody is not None:
        raise ValueError("target= goes with contour=, not with prosody=")
    chunks = [c for u in utterance_chunks for c in u]
    B, n_utt = len(chunks), len(utterance_chunks)
    lens = np.array([len(x) for x in chunks], dtype=np.int32)
    stride = int(lens.max()) if B else 1
    ids = np.zeros((B, stride), dtype=np.int64)
    for b, x in enumerate(chunks):
        ids[b, : len(x)] = x
    uc = np.array([len(u) for u in utterance_chunks], dtype=np.int32)
    fs = None if fixed_steps is None else np.ascontiguousarray([s for u in fixed_steps for s in u], dtype=np.int32)
    mels = (_PF * n_utt)() if want_mels else None
    audios = (_PF * n_utt)()
    nf, ns = (C.c_size_t * n_utt)(), (C.c_size_t * n_utt)()
    head = (tacotron2._h, vocoder._h, _ptr(ids), _ptr(lens), B, stride, _ptr(uc), n_utt, C.byref(opts) if opts else None, None if fs is None else _ptr(fs))
    if contour_at_ids is not None:
        _check(lib.xdtts_synthesize_batch_contour_at_ids(*head, _contour_array(contour_at_ids, n_utt), mels, nf, audios, ns))
    elif target is not None:
        ta, ca, _keep = _target_arrays(target, contour, n_utt)
        _check(lib.xdtts_synthesize_batch_pitch_target(*head, _opt_ref(f0_opts), ta, ca, mels, nf, audios, ns))
    elif contour is not None:
        _check(lib.xdtts_synthesize_batch_contour(*head, _contour_array(contour, n_utt), mels, nf, audios, ns))
    elif prosody is None:
        _check(lib.xdtts_synthesize_batch(*head, mels, nf, audios, ns))
    else:
        _check(lib.xdtts_synthesize_batch_prosody(*head, _prosody_array(prosody, n_utt), mels, nf, audios, ns))
    out_m = [_take(mels[u], N_MEL * nf[u], (N_MEL, nf[u])) for u in range(n_utt)] if want_mels else None
    return out_m, [_take(audios[u], ns[u], (ns[u],)) for u in range(n_utt)]


def synthesize_sequence(tacotron2, vocoder, ids_list, splits_list=None, opts=None, want_mels=True, prosody=None):
    """XdTts::infer (src/lib.rs:110-159) for a sequence of utterances, each decoded alone as `synthesize` does, the vocoder of one
    overlapped with the encoder of the next (xdtts_synthesize_sequence).  Returns (mels or None, audios).  prosody= (a list of
    one Prosody per utterance): what `synthesize(ids_u, prosody=prosody[u])` returns for each (xdtts_synthesize_sequence_prosody)."""
    n = len(ids_list)
    idv = [np.ascontiguousarray(x, dtype=np.int64) for x in ids_list]
    spv = [None if (splits_list is None or splits_list[u] is None) else np.ascontiguousarray(splits_list[u], dtype=np.uintp) for u in range(n)]
    ids_p = (C.c_void_p * n)(*[x.ctypes.data for x in idv])
    n_ids = (C.c_size_t * n)(*[x.size for x in idv])
    sp_p = (C.c_void_p * n)(*[(None if s is None else s.ctypes.data) for s in spv])
    n_sp = (C.c_size_t * n)(*[(0 if s is None else s.size) for s in spv])
    mels = (_PF * n)() if want_mels else None
    audios = (_PF * n)()
    nf, ns = (C.c_size_t * n)(), (C.c_size_t * n)()
    head = (tacotron2._h, vocoder._h, ids_p, n_ids, sp_p, n_sp, n, C.byref(opts) if opts else None)
    if prosody is None:
        _check(lib.xdtts_synthesize_sequence(*head, mels, nf, audios, ns))
    else:
        _check(lib.xdtts_synthesize_sequence_prosody(*head, _prosody_array(prosody, n), mels, nf, audios, ns))
    out_m = [_take(mels[u], N_MEL * nf[u], (N_MEL, nf[u])) for u in range(n)] if want_mels else None
    return out_m, [_take(audios[u], ns[u], (ns[u],)) for u in range(n)]
