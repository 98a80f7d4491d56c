"""ctypes declarations for include/mi_dspu.h (one line per exported symbol)."""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_size_t, c_uint32, c_uint64, c_void_p

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libmi_dspu.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        "libmi_dspu.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` "
        "or `make -C lsp-dsp-units_amd`. There is no CPU fallback." % LIB_PATH)

lib = ctypes.CDLL(LIB_PATH)


class MiError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("mi_dspu error %d: %s" % (code, message))
        self.code = code


class FilterParams(ctypes.Structure):
    """mi_filter_params_t == filter_params_t layout."""
    _fields_ = [("nType", c_uint32), ("nSlope", c_uint32), ("fFreq", c_float), ("fFreq2", c_float),
                ("fGain", c_float), ("fQuality", c_float)]


class FilterCascade(ctypes.Structure):
    _fields_ = [("t", c_float * 4), ("b", c_float * 4)]


class BiquadX1(ctypes.Structure):
    """mi_biquad_x1_t == dsp::biquad_x1_t layout."""
    _fields_ = [(n, c_float) for n in ("b0", "b1", "b2", "a1", "a2", "p0", "p1", "p2")]


class CompressorKnee(ctypes.Structure):
    """mi_compressor_knee_t == dsp::compressor_knee_t layout."""
    _fields_ = [("start", c_float), ("end", c_float), ("gain", c_float), ("herm", c_float * 3), ("tilt", c_float * 2)]


class CompressorParams(ctypes.Structure):
    """mi_compressor_params_t: what Compressor::update_settings computes."""
    _fields_ = [("tau_attack", c_float), ("tau_release", c_float), ("release_threshold", c_float), ("hold", c_uint32),
                ("k", CompressorKnee * 2)]


class CompressorSettings(ctypes.Structure):
    """mi_compressor_settings_t: the values of Compressor's setters."""
    _fields_ = [("sample_rate", c_uint32), ("mode", c_uint32)] + \
               [(n, c_float) for n in ("attack_threshold", "release_threshold", "boost_threshold", "attack", "release",
                                       "hold", "knee", "ratio")]


class ExpanderKnee(ctypes.Structure):
    """mi_expander_knee_t == dsp::expander_knee_t layout."""
    _fields_ = [("start", c_float), ("end", c_float), ("threshold", c_float), ("herm", c_float * 3), ("tilt", c_float * 2)]


class ExpanderParams(ctypes.Structure):
    """mi_expander_params_t: what Expander::update_settings computes."""
    _fields_ = [("tau_attack", c_float), ("tau_release", c_float), ("release_threshold", c_float), ("hold", c_uint32),
                ("k", ExpanderKnee), ("upward", c_uint32)]


class ExpanderSettings(ctypes.Structure):
    """mi_expander_settings_t: the values of Expander's setters."""
    _fields_ = [("sample_rate", c_uint32), ("mode", c_uint32)] + \
               [(n, c_float) for n in ("attack_threshold", "release_threshold", "attack", "release", "hold", "knee", "ratio")]


class GateKnee(ctypes.Structure):
    """mi_gate_knee_t == dsp::gate_knee_t layout."""
    _fields_ = [("start", c_float), ("end", c_float), ("gain_start", c_float), ("gain_end", c_float), ("herm", c_float * 4)]


class GateParams(ctypes.Structure):
    """mi_gate_params_t: what Gate::update_settings computes."""
    _fields_ = [("tau_attack", c_float), ("tau_release", c_float), ("hold", c_uint32), ("reserved", c_uint32), ("k", GateKnee * 2)]


class GateSettings(ctypes.Structure):
    """mi_gate_settings_t: the values of Gate's setters; [0] the open curve, [1] the close curve."""
    _fields_ = [("sample_rate", c_uint32), ("threshold", c_float * 2), ("zone", c_float * 2), ("reduction", c_float),
                ("attack", c_float), ("release", c_float), ("hold", c_float)]


class DynprocDot(ctypes.Structure):
    """mi_dynproc_dot_t == dyndot_t layout."""
    _fields_ = [("input", c_float), ("output", c_float), ("knee", c_float)]


class DynprocSpline(ctypes.Structure):
    """mi_dynproc_spline_t == DynamicProcessor::spline_t layout."""
    _fields_ = [(n, c_float) for n in ("pre_ratio", "post_ratio", "knee_start", "knee_stop", "thresh", "makeup")] + \
               [("herm", c_float * 4)]


class DynprocReaction(ctypes.Structure):
    """mi_dynproc_reaction_t == DynamicProcessor::reaction_t layout."""
    _fields_ = [("level", c_float), ("tau", c_float)]


class DynprocParams(ctypes.Structure):
    """mi_dynproc_params_t: what DynamicProcessor::update_settings computes."""
    _fields_ = [("splines", c_uint32), ("attacks", c_uint32), ("releases", c_uint32), ("hold", c_uint32),
                ("attack", DynprocReaction * 5), ("release", DynprocReaction * 5), ("spline", DynprocSpline * 4)]


class DynprocSettings(ctypes.Structure):
    """mi_dynproc_settings_t: the values of DynamicProcessor's setters."""
    _fields_ = [("sample_rate", c_uint32), ("hold", c_float), ("in_ratio", c_float), ("out_ratio", c_float),
                ("dot", DynprocDot * 4), ("attack_level", c_float * 4), ("release_level", c_float * 4),
                ("attack_time", c_float * 5), ("release_time", c_float * 5)]


class LimiterSettings(ctypes.Structure):
    """mi_limiter_settings_t: the values of Limiter's setters."""
    _fields_ = [("sample_rate", c_uint32), ("mode", c_uint32)] + \
               [(n, c_float) for n in ("threshold", "lookahead", "attack", "release", "knee", "alr_attack", "alr_release", "alr_knee")]


class LimiterParams(ctypes.Structure):
    """mi_limiter_params_t: what Limiter::update_settings computes."""
    _fields_ = [("lookahead", c_uint32), ("mode", c_uint32)] + \
               [(n, ctypes.c_int32) for n in ("attack", "plane", "release", "middle")] + \
               [("v_attack", c_float * 4), ("v_release", c_float * 4)] + \
               [(n, c_float) for n in ("threshold", "ks", "ke", "gain")] + [("hermite", c_float * 3)] + \
               [("tau_attack", c_float), ("tau_release", c_float)]


class AutoGainCurve(ctypes.Structure):
    """mi_autogain_curve_t == AutoGain::compressor_t layout."""
    _fields_ = [(n, c_float) for n in ("x1", "x2", "t", "a", "b", "c", "d")]


class AutoGainSettings(ctypes.Structure):
    """mi_autogain_settings_t: the values of AutoGain's setters."""
    _fields_ = [("sample_rate", c_uint32), ("flags", c_uint32)] + \
               [(n, c_float) for n in ("short_grow", "short_fall", "long_grow", "long_fall", "silence", "deviation", "max_gain")]


class AutoGainParams(ctypes.Structure):
    """mi_autogain_params_t: what AutoGain::update computes, and the values that need no update."""
    _fields_ = [(n, c_float) for n in ("short_kgrow", "short_kfall", "long_kgrow", "long_kfall")] + \
               [("short_comp", AutoGainCurve), ("out_comp", AutoGainCurve)] + \
               [(n, c_float) for n in ("silence", "deviation", "max_gain")] + [("flags", c_uint32)]


class SimpleAutoGainSettings(ctypes.Structure):
    """mi_simple_autogain_settings_t: the values of SimpleAutoGain's setters."""
    _fields_ = [("sample_rate", c_uint32)] + [(n, c_float) for n in ("grow", "fall", "threshold", "min_gain", "max_gain")]


class SimpleAutoGainParams(ctypes.Structure):
    """mi_simple_autogain_params_t: fKGrow, fKFall and the values that need no update."""
    _fields_ = [(n, c_float) for n in ("kgrow", "kfall", "threshold", "min_gain", "max_gain")]


class SidechainParams(ctypes.Structure):
    """mi_sidechain_params_t: what Sidechain::update_settings and set_sample_rate compute, and the settings beside them."""
    _fields_ = [("reactivity", c_uint32), ("tau", c_float), ("interval", c_float), ("capacity", c_uint32), ("mode", c_uint32),
                ("source", c_uint32), ("flags", c_uint32), ("gain", c_float)]


class CorrelometerParams(ctypes.Structure):
    """mi_correlometer_params_t: the period as set, the rings' capacity and the longest period."""
    _fields_ = [("period", c_uint32), ("capacity", c_uint32), ("max_period", c_uint32)]


class CorrelometerState(ctypes.Structure):
    """mi_correlometer_state_t: sCorr, nHead, nWindow."""
    _fields_ = [("v", c_float), ("a", c_float), ("b", c_float), ("head", c_uint32), ("window", c_uint32)]


class PanometerParams(ctypes.Structure):
    """mi_panometer_params_t: the period as set, capacity, the longest period, enPanLaw, fNorm and fDefault."""
    _fields_ = [("period", c_uint32), ("capacity", c_uint32), ("max_period", c_uint32), ("law", c_uint32), ("norm", c_float),
                ("default_pan", c_float)]


class PanometerState(ctypes.Structure):
    """mi_panometer_state_t: fValueA, fValueB, nHead, nWindow."""
    _fields_ = [("value_a", c_float), ("value_b", c_float), ("head", c_uint32), ("window", c_uint32)]


class PeakMeterParams(ctypes.Structure):
    """mi_peakmeter_params_t: fTau, nHold, and the decay factor of process_value() for `count` samples."""
    _fields_ = [("tau", c_float), ("hold", c_uint32), ("factor", c_float), ("count", c_uint32)]


class PeakMeterState(ctypes.Structure):
    """mi_peakmeter_state_t: fPeak, nCounter."""
    _fields_ = [("peak", c_float), ("counter", c_uint32)]


class MeterGraphState(ctypes.Structure):
    """mi_metergraph_state_t: fCurrent, nCount, and the ring's nHead."""
    _fields_ = [("current", c_float), ("count", c_uint32), ("head", c_uint32)]


class MeterGraphParams(ctypes.Structure):
    """mi_metergraph_params_t: enMethod, nPeriod, the ring's nCapacity, fDefault."""
    _fields_ = [("method", c_uint32), ("period", c_uint32), ("frames", c_uint32), ("default_value", c_float)]


class ScaledMeterGraphState(ctypes.Structure):
    """mi_scaled_metergraph_state_t: sHistory's fCurrent, nCount, nHead; sFrames' three and sFrames.nPeriod."""
    _fields_ = [("history_current", c_float), ("history_count", c_uint32), ("history_head", c_uint32), ("frames_current", c_float),
                ("frames_count", c_uint32), ("frames_head", c_uint32), ("frames_period", c_uint32)]


class QuantizedCounterParams(ctypes.Structure):
    """mi_qcounter_params_t: nPeriod, nLevels, fMinValue, fMaxValue, fRStep, bUpdate."""
    _fields_ = [("period", c_uint32), ("levels", c_uint32), ("min_value", c_float), ("max_value", c_float), ("rstep", c_float),
                ("update", c_uint32)]


class QuantizedCounterState(ctypes.Structure):
    """mi_qcounter_state_t: nHead, nCount, nCapacity."""
    _fields_ = [("head", c_uint32), ("count", c_uint32), ("capacity", c_uint32)]


class ScaledMeterGraphParams(ctypes.Structure):
    """mi_scaled_metergraph_params_t: enMethod, nPeriod, nMaxPeriod, sHistory.nPeriod, sFrames.nFrames, sHistory.nFrames."""
    _fields_ = [("method", c_uint32), ("period", c_uint32), ("max_period", c_uint32), ("subsampling", c_uint32), ("frames", c_uint32),
                ("subframes", c_uint32)]


class SurgeParams(ctypes.Structure):
    """mi_surge_params_t: nTransitionMax, nShutdownMax, fOnThreshold, fOffThreshold."""
    _fields_ = [("transition_max", c_uint32), ("shutdown_max", c_uint32), ("on_threshold", c_float), ("off_threshold", c_float)]


class SurgeState(ctypes.Structure):
    """mi_surge_state_t: fGain, nTransitionTime, nShutdownTime, bOn."""
    _fields_ = [("gain", c_float), ("transition_time", c_uint32), ("shutdown_time", c_uint32), ("on", c_uint32)]


class DepopperFade(ctypes.Structure):
    """mi_depopper_fade_t: enMode, fThresh, fTime, fDelay, nSamples, nDelay, fPoly."""
    _fields_ = [("mode", c_uint32), ("threshold", c_float), ("time", c_float), ("delay", c_float), ("samples", ctypes.c_int64),
                ("delay_samples", ctypes.c_int64), ("poly", c_float * 4)]


class DepopperParams(ctypes.Structure):
    """mi_depopper_params_t: both fades, the rate, the maxima, the RMS length and norm, the look and RMS extents, bReconfigure."""
    _fields_ = [("fade_in", DepopperFade), ("fade_out", DepopperFade), ("sample_rate", ctypes.c_uint64), ("look_max", c_float),
                ("rms_max", c_float), ("rms_length", c_float), ("rms_norm", c_float), ("look_min_off", ctypes.c_int64),
                ("look_max_off", ctypes.c_int64), ("look_count", ctypes.c_int64), ("rms_min_off", ctypes.c_int64),
                ("rms_max_off", ctypes.c_int64), ("rms_len", ctypes.c_int64), ("reconfigure", c_uint32)]


class DepopperState(ctypes.Structure):
    """mi_depopper_state_t: fRms, nState, nCounter, nDelay, nRmsOff, nLookOff."""
    _fields_ = [("rms", c_float), ("state", c_uint32), ("counter", ctypes.c_int64), ("delay", ctypes.c_int64),
                ("rms_off", ctypes.c_int64), ("look_off", ctypes.c_int64)]


class BypassState(ctypes.Structure):
    """mi_bypass_state_t: nState (0 on, 1 active, 2 off), fDelta, fGain."""
    _fields_ = [("state", c_uint32), ("delta", c_float), ("gain", c_float)]


class CrossfadeState(ctypes.Structure):
    """mi_crossfade_state_t: nCounter, fDelta, fGain."""
    _fields_ = [("counter", c_uint32), ("delta", c_float), ("gain", c_float)]


class DynDelayState(ctypes.Structure):
    """mi_dyndelay_state_t: nHead."""
    _fields_ = [("head", c_uint32)]


class OscillatorState(ctypes.Structure):
    """mi_oscillator_state_t: nPhaseAcc."""
    _fields_ = [("phase", c_uint32)]


class OscillatorSettings(ctypes.Structure):
    """mi_oscillator_settings_t: the members of one lsp::dspu::Oscillator and what the host knows of its phase."""
    _fields_ = [("function", c_uint32), ("amplitude", c_float), ("frequency", c_float), ("dc_offset", c_float), ("dc_reference", c_uint32),
                ("referenced_dc", c_float), ("init_phase", c_float), ("sample_rate", c_uint64), ("bits", c_uint32), ("mask", c_uint32),
                ("acc2phase", c_float), ("freq_word", c_uint32), ("init_word", c_uint32),
                ("sq_invert", c_uint32), ("sq_amplitude", c_float), ("sq_wave_dc", c_float),
                ("duty", c_float), ("duty_word", c_uint32), ("rect_wave_dc", c_float), ("rect_atten", c_float),
                ("width", c_float), ("width_word", c_uint32), ("saw_coeffs", c_float * 4), ("saw_wave_dc", c_float), ("saw_atten", c_float),
                ("raise_ratio", c_float), ("fall_ratio", c_float), ("points", c_uint32 * 4), ("trap_coeffs", c_float * 4),
                ("trap_wave_dc", c_float), ("trap_atten", c_float),
                ("pos_ratio", c_float), ("neg_ratio", c_float), ("train", c_uint32 * 3), ("pulse_wave_dc", c_float), ("pulse_atten", c_float),
                ("par_invert", c_uint32), ("par_amplitude", c_float), ("par_width", c_float), ("par_word", c_uint32),
                ("par_wave_dc", c_float), ("par_atten", c_float),
                ("oversampling", c_uint32), ("over_mode", c_uint32), ("freq_word_over", c_uint32), ("sync", c_uint32),
                ("phase_known", c_uint32), ("phase", c_uint32), ("unset_rate_ok", c_uint32)]


class AdsrCurve(ctypes.Structure):
    """mi_adsr_curve_t: fTime, fCurve, enFunction and the six floats of gen_params_t."""
    _fields_ = [("time", c_float), ("curve", c_float), ("function", c_uint32), ("params", c_float * 6)]


class AdsrSettings(ctypes.Structure):
    """mi_adsr_settings_t: the members of one lsp::dspu::ADSREnvelope."""
    _fields_ = [("curve", AdsrCurve * 4), ("hold_time", c_float), ("break_level", c_float), ("sustain_level", c_float), ("flags", c_uint32)]


class LcgState(ctypes.Structure):
    """mi_lcg_state_t: the members of one lsp::dspu::Randomizer."""
    _fields_ = [("last", c_uint32 * 4), ("mul1", c_uint32 * 4), ("mul2", c_uint32 * 4), ("add", c_uint32 * 4), ("buf_id", c_uint32)]


class MlsSettings(ctypes.Structure):
    """mi_mls_settings_t: the members of one lsp::dspu::MLS."""
    _fields_ = [(n, c_uint64) for n in ("n_bits", "feedback_bit", "feedback_mask", "active_mask", "taps_mask", "output_mask", "state")] + \
               [("amplitude", c_float), ("offset", c_float), ("sync", c_uint32), ("pad", c_uint32)]


class VelvetState(ctypes.Structure):
    """mi_velvet_state_t: sRandomizer and sMLS of one lsp::dspu::Velvet."""
    _fields_ = [("rand", LcgState), ("pad", c_uint32), ("mls", MlsSettings)]


class SpectralTiltSettings(ctypes.Structure):
    """mi_spectral_tilt_settings_t: the members of one lsp::dspu::SpectralTilt and the sections of its sFilter."""
    _fields_ = [("order", c_uint64), ("sample_rate", c_uint64), ("slope_unit", c_uint32), ("norm", c_uint32),
                ("slope_val", c_float), ("slope_nep_nep", c_float), ("lower_frequency", c_float), ("upper_frequency", c_float),
                ("bypass", c_uint32), ("sync", c_uint32), ("n_sections", c_uint32), ("pad", c_uint32), ("sections", BiquadX1 * 64)]


class NoiseGeneratorSettings(ctypes.Structure):
    """mi_noise_generator_settings_t: the members of one lsp::dspu::NoiseGenerator beside its four units."""
    _fields_ = [(n, c_uint64) for n in ("mls_seed", "velvet_mls_seed", "color_order", "sample_rate", "update")] + \
               [(n, c_uint32) for n in ("mls_n_bits", "lcg_seed", "lcg_distribution", "velvet_rand_seed", "velvet_mls_n_bits", "velvet_core",
                                        "velvet_type", "velvet_crush")] + \
               [(n, c_float) for n in ("velvet_window_width_s", "velvet_arn_delta", "velvet_crush_prob")] + \
               [("color", c_uint32), ("color_slope_unit", c_uint32), ("color_slope", c_float), ("generator", c_uint32), ("inited", c_uint32),
                ("amplitude", c_float), ("offset", c_float)]


class NoiseGeneratorState(ctypes.Structure):
    """mi_noise_generator_state_t: the states of one NoiseGenerator's four units."""
    _fields_ = [("lcg", LcgState), ("pad", c_uint32), ("mls_state", c_uint64), ("mls_n_bits", c_uint64), ("velvet", VelvetState),
                ("filter", c_float * 128)]


# name -> (restype, argtypes); every symbol declared in include/mi_dspu.h must be listed here
# (tests/test_abi.py parses the header and checks both directions).
PROTOTYPES = {
    "mi_dspu_abi_version": (c_int, []),
    "mi_dspu_last_error": (c_char_p, []),
    "mi_dspu_device_count": (c_int, []),
    "mi_dspu_set_device": (c_int, [c_int]),
    "mi_dspu_malloc": (c_int, [POINTER(c_void_p), c_size_t]),
    "mi_dspu_free": (c_int, [c_void_p]),
    "mi_dspu_memset": (c_int, [c_void_p, c_int, c_size_t, c_void_p]),
    "mi_dspu_copy_h2d": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "mi_dspu_copy_d2h": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "mi_dspu_copy_d2d": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "mi_dspu_stream_create": (c_int, [POINTER(c_void_p)]),
    "mi_dspu_stream_destroy": (c_int, [c_void_p]),
    "mi_dspu_stream_synchronize": (c_int, [c_void_p]),
    "mi_dspu_event_create": (c_int, [POINTER(c_void_p)]),
    "mi_dspu_event_destroy": (c_int, [c_void_p]),
    "mi_dspu_event_record": (c_int, [c_void_p, c_void_p]),
    "mi_dspu_event_synchronize": (c_int, [c_void_p]),
    "mi_dspu_event_elapsed_ms": (c_int, [POINTER(c_float), c_void_p, c_void_p]),
    "mi_dspu_profile_next_launch": (c_int, [c_void_p, c_void_p]),
    "mi_dspu_last_launch": (c_char_p, []),
    "mi_dspu_source_sha": (c_char_p, [c_char_p]),
    "mi_dspu_last_stream_clock": (c_int, [POINTER(c_double), POINTER(c_double)]),
    "mi_dspu_graph_begin_capture": (c_int, [c_void_p]),
    "mi_dspu_graph_end_capture": (c_int, [c_void_p, POINTER(c_void_p)]),
    "mi_dspu_graph_launch": (c_int, [c_void_p, c_void_p]),
    "mi_dspu_graph_destroy": (c_int, [c_void_p]),
    "mi_dspu_comm_unique_id": (c_int, [c_void_p]),
    "mi_dspu_comm_create": (c_int, [POINTER(c_void_p), c_void_p, c_int, c_int]),
    "mi_dspu_comm_adopt": (c_int, [POINTER(c_void_p), c_void_p]),
    "mi_dspu_comm_destroy": (c_int, [c_void_p]),
    "mi_dspu_comm_info": (c_int, [c_void_p, POINTER(c_int), POINTER(c_int)]),
    "mi_analyzer_bank_allreduce_bins": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "mi_analyzer_bank_allreduce_bins_begin": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_int, c_void_p]),
    "mi_dspu_comm_wait": (c_int, [c_void_p, c_int, c_void_p]),
    "mi_dynfilter_bank_create": (c_int, [POINTER(c_void_p), c_uint32, c_uint32]),
    "mi_dynfilter_bank_destroy": (c_int, [c_void_p]),
    "mi_dynfilter_bank_set_sample_rate": (c_int, [c_void_p, c_uint32]),
    "mi_dynfilter_bank_set_params": (c_int, [c_void_p, c_uint32, POINTER(FilterParams)]),
    "mi_dynfilter_bank_get_params": (c_int, [c_void_p, c_uint32, POINTER(FilterParams), POINTER(c_int)]),
    "mi_dynfilter_bank_set_filter_active": (c_int, [c_void_p, c_uint32, c_int]),
    "mi_dynfilter_bank_process": (c_int, [c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_dynfilter_sections": (c_int, [POINTER(FilterParams), c_uint32, c_float, POINTER(BiquadX1), c_uint32, POINTER(c_uint32)]),
    "mi_dynfilter_freq_chart": (c_int, [POINTER(FilterParams), c_uint32, c_void_p, c_void_p, c_float, c_size_t]),
    "mi_biquad_bank_create": (c_int, [POINTER(c_void_p), c_uint32, c_uint32]),
    "mi_biquad_bank_destroy": (c_int, [c_void_p]),
    "mi_biquad_bank_set_chains": (c_int, [c_void_p, c_uint32, POINTER(BiquadX1), c_uint32, c_int]),
    "mi_biquad_bank_set_all_chains": (c_int, [c_void_p, POINTER(BiquadX1), c_uint32, c_int]),
    "mi_biquad_bank_size": (c_int, [c_void_p, c_uint32, POINTER(c_uint32)]),
    "mi_biquad_bank_set_row_enabled": (c_int, [c_void_p, c_uint32, c_int]),
    "mi_biquad_bank_set_exact": (c_int, [c_void_p, c_int]),
    "mi_dspu_set_exact_iir_default": (c_int, [c_int]),
    "mi_biquad_bank_commit": (c_int, [c_void_p, c_void_p]),
    "mi_biquad_bank_reset": (c_int, [c_void_p, c_uint32, c_void_p]),
    "mi_biquad_bank_process": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_biquad_bank_process_blocks": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_biquad_bank_impulse_response": (c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p]),
    "mi_biquad_bank_get_state": (c_int, [c_void_p, c_void_p, c_void_p]),
    "mi_biquad_bank_set_state": (c_int, [c_void_p, c_void_p, c_void_p]),
    "mi_filter_design": (c_int, [POINTER(FilterParams), c_uint32, c_void_p, c_uint32, POINTER(c_uint32),
                                 c_void_p, c_uint32, POINTER(c_uint32), POINTER(c_int)]),
    "mi_filter_limit": (c_int, [POINTER(FilterParams), c_uint32]),
    "mi_filter_freq_chart": (c_int, [POINTER(FilterParams), c_uint32, c_void_p, c_void_p, c_size_t]),
    "mi_convolver_bank_create": (c_int, [POINTER(c_void_p), c_uint32, c_void_p, c_size_t, c_void_p, c_uint32, c_uint32,
                                         c_float, c_void_p]),
    "mi_convolver_bank_destroy": (c_int, [c_void_p]),
    "mi_convolver_bank_faults": (c_int, [c_void_p, POINTER(c_uint32), c_void_p]),
    "mi_convolver_bank_reset": (c_int, [c_void_p, c_void_p]),
    "mi_convolver_bank_info": (c_int, [c_void_p, POINTER(c_uint32), POINTER(c_uint32), POINTER(c_uint32),
                                       POINTER(c_uint32)]),
    "mi_convolver_bank_process": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_convolver_bank_process_blocks": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_void_p), c_size_t, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_window": (c_int, [c_void_p, c_size_t, c_int]),
    "mi_window_general": (c_int, [c_void_p, c_size_t, c_int, c_void_p, c_uint32]),
    "mi_envelope_reverse_noise_lin": (c_int, [c_void_p, c_float, c_float, c_float, c_size_t, c_int]),
    "mi_envelope_noise_lin": (c_int, [c_void_p, c_float, c_float, c_float, c_size_t, c_int]),
    "mi_crossover_bank_needs_reconfiguration": (c_int, [c_void_p, POINTER(c_int)]),
    "mi_loudness_bank_needs_update": (c_int, [c_void_p, POINTER(c_int)]),
    "mi_loudness_bank_update_settings": (c_int, [c_void_p, c_void_p]),
    "mi_ilufs_bank_needs_update": (c_int, [c_void_p, POINTER(c_int)]),
    "mi_ilufs_bank_update_settings": (c_int, [c_void_p, c_void_p]),
    "mi_loudness_bank_set_exact": (c_int, [c_void_p, c_int]),
    "mi_ilufs_bank_set_exact": (c_int, [c_void_p, c_int]),
    "mi_analyzer_bank_reset": (c_int, [c_void_p]),
    "mi_envelope_noise_log": (c_int, [c_void_p, c_float, c_float, c_float, c_size_t, c_int, c_int]),
    "mi_envelope_noise_list": (c_int, [c_void_p, c_void_p, c_float, c_size_t, c_int, c_int]),
    "mi_spectral_bank_create": (c_int, [POINTER(c_void_p), c_uint32, c_uint32]),
    "mi_spectral_bank_destroy": (c_int, [c_void_p]),
    "mi_spectral_bank_set_rank": (c_int, [c_void_p, c_uint32]),
    "mi_spectral_bank_set_phase": (c_int, [c_void_p, c_float]),
    "mi_spectral_bank_get": (c_int, [c_void_p, POINTER(c_uint32), POINTER(c_uint32), POINTER(c_uint32)]),
    "mi_spectral_bank_bind": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "mi_spectral_bank_unbind": (c_int, [c_void_p]),
    "mi_spectral_bank_bind_mask": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "mi_spectral_bank_bind_channels": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "mi_spectral_bank_reset": (c_int, [c_void_p, c_void_p]),
    "mi_spectral_bank_process": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_spectral_bank_process_blocks": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_void_p), c_size_t, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_spectral_bank_set_timing": (c_int, [c_void_p, c_int]),
    "mi_analyzer_bank_create": (c_int, [POINTER(c_void_p), c_uint32, c_uint32, c_uint32, c_float, c_uint32]),
    "mi_analyzer_bank_destroy": (c_int, [c_void_p]),
    "mi_analyzer_bank_configure": (c_int, [c_void_p, c_int, ctypes.c_double]),
    "mi_analyzer_bank_channel": (c_int, [c_void_p, c_uint32, c_int, c_uint32]),
    "mi_analyzer_bank_process": (c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p]),
    "mi_analyzer_bank_get_spectrum": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p, c_uint32, c_void_p]),
    "mi_analyzer_bank_reduce_bins": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    "mi_analyzer_bank_process_reduce": (c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p, c_int, c_void_p]),
    "mi_analyzer_bank_process_reduce_frames": (c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_void_p, c_size_t, c_int, c_void_p]),
    "mi_analyzer_bank_info": (c_int, [c_void_p, POINTER(c_uint32), POINTER(c_uint32), POINTER(c_uint32), POINTER(c_uint32)]),
    "mi_convolver_bank_set_irs_device": (c_int, [c_void_p, c_void_p, c_size_t, c_uint32, c_void_p, c_void_p]),
    "mi_convolver_bank_crossfade_irs_device": (c_int, [c_void_p, c_void_p, c_size_t, c_uint32, c_void_p, c_void_p]),
    "mi_spectral_bank_set_windows": (c_int, [c_void_p, c_int, c_int]),
    "mi_equalizer_bank_create": (c_int, [POINTER(c_void_p), c_uint32, c_uint32, c_uint32]),
    "mi_equalizer_bank_destroy": (c_int, [c_void_p]),
    "mi_equalizer_bank_set_params": (c_int, [c_void_p, c_uint32, c_uint32, POINTER(FilterParams)]),
    "mi_equalizer_bank_get_params": (c_int, [c_void_p, c_uint32, c_uint32, POINTER(FilterParams)]),
    "mi_equalizer_bank_set_mode": (c_int, [c_void_p, c_int]),
    "mi_equalizer_bank_set_sample_rate": (c_int, [c_void_p, c_uint32]),
    "mi_equalizer_bank_set_actual_sample_rate": (c_int, [c_void_p, c_uint32]),
    "mi_equalizer_bank_get_latency": (c_int, [c_void_p, POINTER(c_uint32), c_void_p]),
    "mi_equalizer_bank_set_smooth": (c_int, [c_void_p, c_int]),
    "mi_loudness_bank_create": (c_int, [POINTER(c_void_p), c_uint32, c_uint32, c_float]),
    "mi_loudness_bank_destroy": (c_int, [c_void_p]),
    "mi_loudness_bank_set_sample_rate": (c_int, [c_void_p, c_uint32, c_void_p]),
    "mi_loudness_bank_set_period": (c_int, [c_void_p, c_float]),
    "mi_loudness_bank_set_weighting": (c_int, [c_void_p, c_int]),
    "mi_loudness_bank_set_designation": (c_int, [c_void_p, c_uint32, c_int]),
    "mi_loudness_bank_set_link": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_loudness_bank_set_active": (c_int, [c_void_p, c_uint32, c_int, c_void_p]),
    "mi_loudness_bank_clear": (c_int, [c_void_p, c_void_p]),
    "mi_loudness_bank_set_bound": (c_int, [c_void_p, c_uint32, c_int]),
    "mi_loudness_bank_latency": (c_int, [c_void_p, POINTER(c_uint32)]),
    "mi_loudness_bank_process": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_loudness_bank_process_gain": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_float, c_void_p]),
    "mi_loudness_bank_loudness": (c_int, [c_void_p, POINTER(c_float), c_void_p]),
    "mi_ilufs_bank_create": (c_int, [POINTER(c_void_p), c_uint32, c_uint32, c_float, c_float]),
    "mi_ilufs_bank_destroy": (c_int, [c_void_p]),
    "mi_ilufs_bank_set_sample_rate": (c_int, [c_void_p, c_uint32, c_void_p]),
    "mi_ilufs_bank_set_integration_period": (c_int, [c_void_p, c_float, c_void_p]),
    "mi_ilufs_bank_set_weighting": (c_int, [c_void_p, c_int]),
    "mi_ilufs_bank_set_designation": (c_int, [c_void_p, c_uint32, c_int]),
    "mi_ilufs_bank_set_active": (c_int, [c_void_p, c_uint32, c_int]),
    "mi_ilufs_bank_clear": (c_int, [c_void_p, c_void_p]),
    "mi_ilufs_bank_process": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_float, c_void_p]),
    "mi_ilufs_bank_loudness": (c_int, [c_void_p, POINTER(c_float), c_void_p]),
    "mi_ilufs_bank_history": (c_int, [c_void_p, c_void_p, POINTER(c_uint32), POINTER(c_uint32), POINTER(c_uint32), c_void_p]),
    "mi_truepeak_bank_create": (c_int, [POINTER(c_void_p), c_uint32]),
    "mi_truepeak_bank_destroy": (c_int, [c_void_p]),
    "mi_truepeak_bank_set_sample_rate": (c_int, [c_void_p, c_uint32]),
    "mi_truepeak_bank_update_settings": (c_int, [c_void_p, c_void_p]),
    "mi_truepeak_bank_clear": (c_int, [c_void_p, c_void_p]),
    "mi_truepeak_bank_latency": (c_int, [c_void_p, POINTER(c_uint32)]),
    "mi_truepeak_bank_oversampling": (c_int, [c_void_p, POINTER(c_uint32)]),
    "mi_truepeak_bank_process": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_truepeak_bank_process_max": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_void_p]),
    "mi_truepeak_coefficients": (c_int, [c_uint32, POINTER(c_float), POINTER(c_size_t)]),
    "mi_oversampler_bank_create": (c_int, [POINTER(c_void_p), c_uint32]),
    "mi_oversampler_bank_destroy": (c_int, [c_void_p]),
    "mi_oversampler_bank_set_sample_rate": (c_int, [c_void_p, c_uint32]),
    "mi_oversampler_bank_set_mode": (c_int, [c_void_p, c_uint32]),
    "mi_oversampler_bank_mode": (c_int, [c_void_p, POINTER(c_uint32)]),
    "mi_oversampler_bank_set_filtering": (c_int, [c_void_p, c_int]),
    "mi_oversampler_bank_filtering": (c_int, [c_void_p, POINTER(c_int)]),
    "mi_oversampler_bank_modified": (c_int, [c_void_p, POINTER(c_int)]),
    "mi_oversampler_bank_update_settings": (c_int, [c_void_p, c_void_p]),
    "mi_oversampler_bank_oversampling": (c_int, [c_void_p, POINTER(c_uint32)]),
    "mi_oversampler_bank_latency": (c_int, [c_void_p, POINTER(c_uint32)]),
    "mi_oversampler_bank_max_latency": (c_int, [c_void_p, POINTER(c_uint32)]),
    "mi_oversampler_bank_reserve": (c_int, [c_void_p, c_size_t]),
    "mi_oversampler_bank_set_exact": (c_int, [c_void_p, c_int]),
    "mi_oversampler_bank_upsample": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_oversampler_bank_downsample": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_oversampler_bank_process": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p]),
    "mi_oversampler_bank_get_filter": (c_int, [c_void_p, POINTER(FilterParams), POINTER(c_uint32)]),
    "mi_oversampler_coefficients": (c_int, [c_uint32, POINTER(c_float), POINTER(c_size_t)]),
    "mi_compressor_compute_params": (c_int, [POINTER(CompressorSettings), POINTER(CompressorParams)]),
    "mi_compressor_bank_create": (c_int, [POINTER(c_void_p), c_uint32]),
    "mi_compressor_bank_destroy": (c_int, [c_void_p]),
    "mi_compressor_bank_set_sample_rate": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_compressor_bank_set_mode": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_compressor_bank_set_threshold": (c_int, [c_void_p, c_uint32, c_float, c_float]),
    "mi_compressor_bank_set_boost_threshold": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_compressor_bank_set_timings": (c_int, [c_void_p, c_uint32, c_float, c_float]),
    "mi_compressor_bank_set_hold": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_compressor_bank_set_knee": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_compressor_bank_set_ratio": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_compressor_bank_update_settings": (c_int, [c_void_p, c_void_p]),
    "mi_compressor_bank_clear": (c_int, [c_void_p, c_void_p]),
    "mi_compressor_bank_get_params": (c_int, [c_void_p, c_uint32, POINTER(CompressorParams)]),
    "mi_compressor_bank_get_state": (c_int, [c_void_p, c_uint32, POINTER(c_float), POINTER(c_float), POINTER(c_uint32), c_void_p]),
    "mi_compressor_bank_process": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_compressor_bank_process_apply": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_compressor_bank_curve": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_expander_compute_params": (c_int, [POINTER(ExpanderSettings), POINTER(ExpanderParams)]),
    "mi_expander_bank_create": (c_int, [POINTER(c_void_p), c_uint32]),
    "mi_expander_bank_destroy": (c_int, [c_void_p]),
    "mi_expander_bank_set_sample_rate": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_expander_bank_set_mode": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_expander_bank_set_threshold": (c_int, [c_void_p, c_uint32, c_float, c_float]),
    "mi_expander_bank_set_timings": (c_int, [c_void_p, c_uint32, c_float, c_float]),
    "mi_expander_bank_set_hold": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_expander_bank_set_knee": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_expander_bank_set_ratio": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_expander_bank_update_settings": (c_int, [c_void_p, c_void_p]),
    "mi_expander_bank_clear": (c_int, [c_void_p, c_void_p]),
    "mi_expander_bank_get_params": (c_int, [c_void_p, c_uint32, POINTER(ExpanderParams)]),
    "mi_expander_bank_get_state": (c_int, [c_void_p, c_uint32, POINTER(c_float), POINTER(c_float), POINTER(c_uint32), c_void_p]),
    "mi_expander_bank_process": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_expander_bank_process_apply": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_expander_bank_curve": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_gate_compute_params": (c_int, [POINTER(GateSettings), POINTER(GateParams)]),
    "mi_gate_bank_create": (c_int, [POINTER(c_void_p), c_uint32]),
    "mi_gate_bank_destroy": (c_int, [c_void_p]),
    "mi_gate_bank_set_sample_rate": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_gate_bank_set_threshold": (c_int, [c_void_p, c_uint32, c_float, c_float]),
    "mi_gate_bank_set_zone": (c_int, [c_void_p, c_uint32, c_float, c_float]),
    "mi_gate_bank_set_reduction": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_gate_bank_set_timings": (c_int, [c_void_p, c_uint32, c_float, c_float]),
    "mi_gate_bank_set_hold": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_gate_bank_update_settings": (c_int, [c_void_p, c_void_p]),
    "mi_gate_bank_clear": (c_int, [c_void_p, c_void_p]),
    "mi_gate_bank_get_params": (c_int, [c_void_p, c_uint32, POINTER(GateParams)]),
    "mi_gate_bank_get_state": (c_int, [c_void_p, c_uint32, POINTER(c_float), POINTER(c_float), POINTER(c_uint32), POINTER(c_uint32), c_void_p]),
    "mi_gate_bank_process": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_gate_bank_process_apply": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_gate_bank_curve": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_size_t, c_size_t, c_void_p]),
    "mi_dynproc_compute_params": (c_int, [POINTER(DynprocSettings), POINTER(DynprocParams)]),
    "mi_dynproc_bank_create": (c_int, [POINTER(c_void_p), c_uint32]),
    "mi_dynproc_bank_destroy": (c_int, [c_void_p]),
    "mi_dynproc_bank_set_sample_rate": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_dynproc_bank_set_in_ratio": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_dynproc_bank_set_out_ratio": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_dynproc_bank_set_dot": (c_int, [c_void_p, c_uint32, c_uint32, POINTER(DynprocDot)]),
    "mi_dynproc_bank_set_attack_level": (c_int, [c_void_p, c_uint32, c_uint32, c_float]),
    "mi_dynproc_bank_set_release_level": (c_int, [c_void_p, c_uint32, c_uint32, c_float]),
    "mi_dynproc_bank_set_attack_time": (c_int, [c_void_p, c_uint32, c_uint32, c_float]),
    "mi_dynproc_bank_set_release_time": (c_int, [c_void_p, c_uint32, c_uint32, c_float]),
    "mi_dynproc_bank_set_hold": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_dynproc_bank_update_settings": (c_int, [c_void_p, c_void_p]),
    "mi_dynproc_bank_clear": (c_int, [c_void_p, c_void_p]),
    "mi_dynproc_bank_get_params": (c_int, [c_void_p, c_uint32, POINTER(DynprocParams)]),
    "mi_dynproc_bank_get_state": (c_int, [c_void_p, c_uint32, POINTER(c_float), POINTER(c_float), POINTER(c_uint32), c_void_p]),
    "mi_dynproc_bank_process": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_dynproc_bank_process_apply": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_dynproc_bank_curve": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_dynproc_bank_model": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_limiter_compute_params": (c_int, [POINTER(LimiterSettings), POINTER(LimiterParams)]),
    "mi_limiter_compute_patch": (c_int, [POINTER(LimiterParams), c_void_p, c_size_t]),
    "mi_limiter_bank_create": (c_int, [POINTER(c_void_p), c_uint32, c_uint32, c_float]),
    "mi_limiter_bank_destroy": (c_int, [c_void_p]),
    "mi_limiter_bank_set_sample_rate": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_limiter_bank_set_mode": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_limiter_bank_set_threshold": (c_int, [c_void_p, c_uint32, c_float, c_int]),
    "mi_limiter_bank_set_attack": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_limiter_bank_set_release": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_limiter_bank_set_lookahead": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_limiter_bank_set_knee": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_limiter_bank_set_alr": (c_int, [c_void_p, c_uint32, c_int]),
    "mi_limiter_bank_set_alr_attack": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_limiter_bank_set_alr_release": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_limiter_bank_set_alr_knee": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_limiter_bank_update_settings": (c_int, [c_void_p, c_void_p]),
    "mi_limiter_bank_clear": (c_int, [c_void_p, c_void_p]),
    "mi_limiter_bank_get_params": (c_int, [c_void_p, c_uint32, POINTER(LimiterParams)]),
    "mi_limiter_bank_get_patch": (c_int, [c_void_p, c_uint32, c_void_p, c_size_t, POINTER(c_uint32), c_void_p]),
    "mi_limiter_bank_get_latency": (c_int, [c_void_p, c_uint32, POINTER(c_uint32)]),
    "mi_limiter_bank_get_state": (c_int, [c_void_p, c_uint32, POINTER(c_uint32), POINTER(c_float), POINTER(c_uint32), POINTER(c_uint32),
                                          POINTER(c_uint32), c_void_p]),
    "mi_limiter_bank_process": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_limiter_bank_process_apply": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_autogain_compute_params": (c_int, [POINTER(AutoGainSettings), POINTER(AutoGainParams)]),
    "mi_autogain_bank_create": (c_int, [POINTER(c_void_p), c_uint32]),
    "mi_autogain_bank_destroy": (c_int, [c_void_p]),
    "mi_autogain_bank_set_sample_rate": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_autogain_bank_set_silence_threshold": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_autogain_bank_set_deviation": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_autogain_bank_set_short_grow": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_autogain_bank_set_short_fall": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_autogain_bank_set_short_speed": (c_int, [c_void_p, c_uint32, c_float, c_float]),
    "mi_autogain_bank_set_long_grow": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_autogain_bank_set_long_fall": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_autogain_bank_set_long_speed": (c_int, [c_void_p, c_uint32, c_float, c_float]),
    "mi_autogain_bank_set_max_gain": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_autogain_bank_set_max_gain_control": (c_int, [c_void_p, c_uint32, c_float, c_int]),
    "mi_autogain_bank_enable_max_gain": (c_int, [c_void_p, c_uint32, c_int]),
    "mi_autogain_bank_enable_quick_amplifier": (c_int, [c_void_p, c_uint32, c_int]),
    "mi_autogain_bank_update_settings": (c_int, [c_void_p, c_void_p]),
    "mi_autogain_bank_get_params": (c_int, [c_void_p, c_uint32, POINTER(AutoGainParams)]),
    "mi_autogain_bank_get_state": (c_int, [c_void_p, c_uint32, POINTER(c_float), POINTER(c_float), POINTER(c_uint32), c_void_p]),
    "mi_autogain_bank_process": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_size_t,
                                         c_size_t, c_void_p]),
    "mi_autogain_bank_process_level": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t,
                                               c_size_t, c_void_p]),
    "mi_autogain_bank_process_apply": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t,
                                               c_size_t, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_simple_autogain_compute_params": (c_int, [POINTER(SimpleAutoGainSettings), POINTER(SimpleAutoGainParams)]),
    "mi_simple_autogain_bank_create": (c_int, [POINTER(c_void_p), c_uint32]),
    "mi_simple_autogain_bank_destroy": (c_int, [c_void_p]),
    "mi_simple_autogain_bank_set_sample_rate": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_simple_autogain_bank_set_grow": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_simple_autogain_bank_set_fall": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_simple_autogain_bank_set_speed": (c_int, [c_void_p, c_uint32, c_float, c_float]),
    "mi_simple_autogain_bank_set_max_gain": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_simple_autogain_bank_set_min_gain": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_simple_autogain_bank_set_gain": (c_int, [c_void_p, c_uint32, c_float, c_float]),
    "mi_simple_autogain_bank_set_threshold": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_simple_autogain_bank_update_settings": (c_int, [c_void_p, c_void_p]),
    "mi_simple_autogain_bank_get_params": (c_int, [c_void_p, c_uint32, POINTER(SimpleAutoGainParams)]),
    "mi_simple_autogain_bank_get_state": (c_int, [c_void_p, c_uint32, POINTER(c_float), c_void_p]),
    "mi_simple_autogain_bank_process": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_sidechain_compute_params": (c_int, [c_uint32, c_float, c_float, POINTER(SidechainParams)]),
    "mi_sidechain_bank_create": (c_int, [POINTER(c_void_p), c_uint32, c_uint32, c_float]),
    "mi_sidechain_bank_destroy": (c_int, [c_void_p]),
    "mi_sidechain_bank_set_sample_rate": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_sidechain_bank_set_reactivity": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_sidechain_bank_set_stereo_mode": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_sidechain_bank_set_source": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_sidechain_bank_set_mode": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_sidechain_bank_set_gain": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_sidechain_bank_clear": (c_int, [c_void_p, c_uint32]),
    "mi_sidechain_bank_update_settings": (c_int, [c_void_p, c_void_p]),
    "mi_sidechain_bank_get_params": (c_int, [c_void_p, c_uint32, POINTER(SidechainParams)]),
    "mi_sidechain_bank_get_state": (c_int, [c_void_p, c_uint32, POINTER(c_float), POINTER(c_uint32), POINTER(c_uint32), c_void_p]),
    "mi_sidechain_bank_process": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_sidechain_bank_premix": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_sidechain_bank_process_premixed": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_correlometer_bank_create": (c_int, [POINTER(c_void_p), c_uint32, c_uint32]),
    "mi_correlometer_bank_destroy": (c_int, [c_void_p]),
    "mi_correlometer_bank_set_period": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_correlometer_bank_clear": (c_int, [c_void_p, c_uint32]),
    "mi_correlometer_bank_update_settings": (c_int, [c_void_p, c_void_p]),
    "mi_correlometer_bank_get_params": (c_int, [c_void_p, c_uint32, POINTER(CorrelometerParams)]),
    "mi_correlometer_bank_get_state": (c_int, [c_void_p, c_uint32, POINTER(CorrelometerState), c_void_p]),
    "mi_correlometer_bank_set_state": (c_int, [c_void_p, c_uint32, POINTER(CorrelometerState), c_uint32, c_void_p]),
    "mi_correlometer_bank_process": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_panometer_bank_create": (c_int, [POINTER(c_void_p), c_uint32, c_uint32]),
    "mi_panometer_bank_destroy": (c_int, [c_void_p]),
    "mi_panometer_bank_set_period": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_panometer_bank_set_pan_law": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_panometer_bank_set_default_pan": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_panometer_bank_clear": (c_int, [c_void_p, c_uint32]),
    "mi_panometer_bank_update_settings": (c_int, [c_void_p, c_void_p]),
    "mi_panometer_bank_get_params": (c_int, [c_void_p, c_uint32, POINTER(PanometerParams)]),
    "mi_panometer_bank_get_state": (c_int, [c_void_p, c_uint32, POINTER(PanometerState), c_void_p]),
    "mi_panometer_bank_set_state": (c_int, [c_void_p, c_uint32, POINTER(PanometerState), c_uint32, c_void_p]),
    "mi_panometer_bank_process": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_peakmeter_compute_params": (c_int, [c_uint32, c_float, c_float, POINTER(PeakMeterParams)]),
    "mi_peakmeter_bank_create": (c_int, [POINTER(c_void_p), c_uint32]),
    "mi_peakmeter_bank_destroy": (c_int, [c_void_p]),
    "mi_peakmeter_bank_set_sample_rate": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_peakmeter_bank_set_hold_time": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_peakmeter_bank_set_release_time": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_peakmeter_bank_set_time": (c_int, [c_void_p, c_uint32, c_float, c_float]),
    "mi_peakmeter_bank_clear": (c_int, [c_void_p, c_uint32]),
    "mi_peakmeter_bank_update_settings": (c_int, [c_void_p, c_void_p]),
    "mi_peakmeter_bank_get_params": (c_int, [c_void_p, c_uint32, POINTER(PeakMeterParams)]),
    "mi_peakmeter_bank_set_params": (c_int, [c_void_p, c_uint32, POINTER(PeakMeterParams)]),
    "mi_peakmeter_bank_get_state": (c_int, [c_void_p, c_uint32, POINTER(PeakMeterState), c_void_p]),
    "mi_peakmeter_bank_set_state": (c_int, [c_void_p, c_uint32, POINTER(PeakMeterState), c_void_p]),
    "mi_peakmeter_bank_process": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_peakmeter_bank_process_value": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "mi_surge_bank_create": (c_int, [POINTER(c_void_p), c_uint32]),
    "mi_surge_bank_destroy": (c_int, [c_void_p]),
    "mi_surge_bank_set_transition_time": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_surge_bank_set_shutdown_time": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_surge_bank_set_on_threshold": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_surge_bank_set_off_threshold": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_surge_bank_set_threshold": (c_int, [c_void_p, c_uint32, c_float, c_float]),
    "mi_surge_bank_reset": (c_int, [c_void_p, c_uint32]),
    "mi_surge_bank_get_params": (c_int, [c_void_p, c_uint32, POINTER(SurgeParams)]),
    "mi_surge_bank_get_state": (c_int, [c_void_p, c_uint32, POINTER(SurgeState), c_void_p]),
    "mi_surge_bank_set_state": (c_int, [c_void_p, c_uint32, POINTER(SurgeState), c_void_p]),
    "mi_surge_bank_process": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_surge_bank_process_mul": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_depopper_compute_params": (c_int, [POINTER(DepopperParams), POINTER(DepopperParams), c_void_p, c_size_t, c_void_p, c_size_t]),
    "mi_depopper_compute_extents": (c_int, [ctypes.c_uint64, c_float, c_float, POINTER(DepopperParams)]),
    "mi_depopper_square_threshold": (c_int, [c_float, POINTER(c_float)]),
    "mi_depopper_bank_create": (c_int, [POINTER(c_void_p), c_uint32]),
    "mi_depopper_bank_destroy": (c_int, [c_void_p]),
    "mi_depopper_bank_init": (c_int, [c_void_p, c_uint32, ctypes.c_uint64, c_float, c_float]),
    "mi_depopper_bank_set_fade_in_mode": (c_int, [c_void_p, c_uint32, c_uint32, POINTER(c_uint32)]),
    "mi_depopper_bank_set_fade_out_mode": (c_int, [c_void_p, c_uint32, c_uint32, POINTER(c_uint32)]),
    "mi_depopper_bank_set_fade_in_time": (c_int, [c_void_p, c_uint32, c_float, POINTER(c_float)]),
    "mi_depopper_bank_set_fade_out_time": (c_int, [c_void_p, c_uint32, c_float, POINTER(c_float)]),
    "mi_depopper_bank_set_fade_in_threshold": (c_int, [c_void_p, c_uint32, c_float, POINTER(c_float)]),
    "mi_depopper_bank_set_fade_out_threshold": (c_int, [c_void_p, c_uint32, c_float, POINTER(c_float)]),
    "mi_depopper_bank_set_fade_in_delay": (c_int, [c_void_p, c_uint32, c_float, POINTER(c_float)]),
    "mi_depopper_bank_set_fade_out_delay": (c_int, [c_void_p, c_uint32, c_float, POINTER(c_float)]),
    "mi_depopper_bank_set_rms_length": (c_int, [c_void_p, c_uint32, c_float, POINTER(c_float)]),
    "mi_depopper_bank_set_settings": (c_int, [c_void_p, c_uint32, POINTER(DepopperParams)]),
    "mi_depopper_bank_update_settings": (c_int, [c_void_p, c_void_p]),
    "mi_depopper_bank_get_params": (c_int, [c_void_p, c_uint32, POINTER(DepopperParams)]),
    "mi_depopper_bank_get_fade_table": (c_int, [c_void_p, c_uint32, c_uint32, c_void_p, c_size_t, POINTER(c_size_t)]),
    "mi_depopper_bank_latency": (c_int, [c_void_p, c_uint32, POINTER(ctypes.c_int64)]),
    "mi_depopper_bank_get_state": (c_int, [c_void_p, c_uint32, POINTER(DepopperState), c_void_p, c_void_p, c_void_p]),
    "mi_depopper_bank_set_state": (c_int, [c_void_p, c_uint32, POINTER(DepopperState), c_void_p, c_void_p, c_void_p]),
    "mi_depopper_bank_process": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_bypass_bank_create": (c_int, [POINTER(c_void_p), c_uint32]),
    "mi_bypass_bank_destroy": (c_int, [c_void_p]),
    "mi_bypass_bank_init": (c_int, [c_void_p, c_uint32, c_int, c_float]),
    "mi_bypass_bank_set_bypass": (c_int, [c_void_p, c_uint32, c_int, POINTER(c_int)]),
    "mi_bypass_bank_bypassing": (c_int, [c_void_p, c_uint32, POINTER(c_int), c_void_p]),
    "mi_bypass_bank_get_state": (c_int, [c_void_p, c_uint32, POINTER(BypassState), c_void_p]),
    "mi_bypass_bank_set_state": (c_int, [c_void_p, c_uint32, POINTER(BypassState), c_void_p]),
    "mi_bypass_bank_process": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_bypass_bank_process_wet": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_size_t, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_bypass_bank_process_drywet": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_size_t, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_crossfade_bank_create": (c_int, [POINTER(c_void_p), c_uint32]),
    "mi_crossfade_bank_destroy": (c_int, [c_void_p]),
    "mi_crossfade_bank_init": (c_int, [c_void_p, c_uint32, c_int, c_float]),
    "mi_crossfade_bank_toggle": (c_int, [c_void_p, c_uint32, POINTER(c_int)]),
    "mi_crossfade_bank_reset": (c_int, [c_void_p, c_uint32]),
    "mi_crossfade_bank_remaining": (c_int, [c_void_p, c_uint32, POINTER(c_size_t)]),
    "mi_crossfade_bank_get_state": (c_int, [c_void_p, c_uint32, POINTER(CrossfadeState), c_void_p]),
    "mi_crossfade_bank_set_state": (c_int, [c_void_p, c_uint32, POINTER(CrossfadeState), c_void_p]),
    "mi_crossfade_bank_process": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_splitter_bank_create": (c_int, [POINTER(c_void_p), c_uint32, c_uint32, c_uint32]),
    "mi_splitter_bank_destroy": (c_int, [c_void_p]),
    "mi_splitter_bank_set_rank": (c_int, [c_void_p, c_uint32]),
    "mi_splitter_bank_set_chunk_rank": (c_int, [c_void_p, ctypes.c_int32]),
    "mi_splitter_bank_set_phase": (c_int, [c_void_p, c_float]),
    "mi_splitter_bank_get": (c_int, [c_void_p, POINTER(c_uint32), POINTER(c_uint32), POINTER(c_uint32), POINTER(c_uint32)]),
    "mi_splitter_bank_bind_copy": (c_int, [c_void_p, c_uint32, c_void_p]),
    "mi_splitter_bank_bind_mask": (c_int, [c_void_p, c_uint32, POINTER(c_float), c_size_t, c_void_p]),
    "mi_splitter_bank_bind_callback": (c_int, [c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mi_splitter_bank_unbind": (c_int, [c_void_p, c_uint32]),
    "mi_splitter_bank_clear": (c_int, [c_void_p, c_void_p]),
    "mi_splitter_bank_process": (c_int, [c_void_p, POINTER(c_void_p), c_void_p, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_splitter_bank_process_blocks": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_void_p), c_size_t, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_crossover_hipass": (c_float, [c_float, c_float, c_float]),
    "mi_crossover_lopass": (c_float, [c_float, c_float, c_float]),
    "mi_crossover_hipass_set": (None, [POINTER(c_float), POINTER(c_float), c_float, c_float, c_size_t]),
    "mi_crossover_hipass_apply": (None, [POINTER(c_float), POINTER(c_float), c_float, c_float, c_size_t]),
    "mi_crossover_lopass_set": (None, [POINTER(c_float), POINTER(c_float), c_float, c_float, c_size_t]),
    "mi_crossover_lopass_apply": (None, [POINTER(c_float), POINTER(c_float), c_float, c_float, c_size_t]),
    "mi_crossover_hipass_fft_set": (None, [POINTER(c_float), c_float, c_float, c_float, c_size_t]),
    "mi_crossover_hipass_fft_apply": (None, [POINTER(c_float), c_float, c_float, c_float, c_size_t]),
    "mi_crossover_lopass_fft_set": (None, [POINTER(c_float), c_float, c_float, c_float, c_size_t]),
    "mi_crossover_lopass_fft_apply": (None, [POINTER(c_float), c_float, c_float, c_float, c_size_t]),
    "mi_crossover_bank_create": (c_int, [POINTER(c_void_p), c_uint32, c_uint32]),
    "mi_crossover_bank_destroy": (c_int, [c_void_p]),
    "mi_crossover_bank_set_sample_rate": (c_int, [c_void_p, c_uint32]),
    "mi_crossover_bank_set_slope": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_crossover_bank_set_frequency": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_crossover_bank_set_mode": (c_int, [c_void_p, c_uint32, c_int]),
    "mi_crossover_bank_set_gain": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_crossover_bank_get_split": (c_int, [c_void_p, c_uint32, POINTER(c_uint32), POINTER(c_float), POINTER(c_int)]),
    "mi_crossover_bank_get_band": (c_int, [c_void_p, c_uint32, POINTER(c_float), POINTER(c_float), POINTER(c_float), POINTER(c_int), c_void_p]),
    "mi_crossover_bank_process": (c_int, [c_void_p, POINTER(c_void_p), c_void_p, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_crossover_bank_process_blocks": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_void_p), c_size_t, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_crossover_bank_freq_chart": (c_int, [c_void_p, c_uint32, POINTER(c_float), POINTER(c_float), c_size_t, c_void_p]),
    "mi_equalizer_bank_reset": (c_int, [c_void_p, c_void_p]),
    "mi_equalizer_bank_process": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_equalizer_bank_process_blocks": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_equalizer_bank_info": (c_int, [c_void_p, POINTER(c_uint32), POINTER(c_uint32), POINTER(c_int), POINTER(c_uint32)]),
    "mi_dyndelay_bank_create": (c_int, [POINTER(c_void_p), c_uint32, c_size_t]),
    "mi_dyndelay_bank_destroy": (c_int, [c_void_p]),
    "mi_dyndelay_bank_get": (c_int, [c_void_p, c_uint32, POINTER(c_uint32), POINTER(c_uint32), POINTER(c_uint32)]),
    "mi_dyndelay_bank_get_state": (c_int, [c_void_p, c_uint32, POINTER(DynDelayState), c_void_p]),
    "mi_dyndelay_bank_set_state": (c_int, [c_void_p, c_uint32, POINTER(DynDelayState), c_void_p]),
    "mi_dyndelay_bank_clear": (c_int, [c_void_p, c_void_p]),
    "mi_dyndelay_bank_process": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_size_t,
                                         c_size_t, c_size_t, c_void_p]),
    "mi_dyndelay_bank_copy": (c_int, [c_void_p, c_uint32, c_void_p, c_uint32, c_void_p]),
    "mi_dyndelay_bank_read_line": (c_int, [c_void_p, c_uint32, c_void_p, c_size_t, c_size_t, c_void_p]),
    "mi_dyndelay_bank_write_line": (c_int, [c_void_p, c_uint32, c_void_p, c_size_t, c_size_t, c_void_p]),
    "mi_dyndelay_bank_count_steps": (c_int, [c_void_p, c_int, c_void_p]),
    "mi_dyndelay_bank_steps": (c_int, [c_void_p, POINTER(c_uint64), POINTER(c_uint64), c_void_p]),
    "mi_adsr_settings_init": (c_int, [POINTER(AdsrSettings)]),
    "mi_adsr_settings_set": (c_int, [POINTER(AdsrSettings), c_uint32, c_double, c_double, c_double]),
    "mi_adsr_settings_update": (c_int, [POINTER(AdsrSettings)]),
    "mi_adsr_settings_process": (c_int, [POINTER(AdsrSettings), c_float, POINTER(c_float)]),
    "mi_interpolation_hermite_cubic": (c_int, [c_void_p] + [c_float] * 6),
    "mi_interpolation_hermite_quadro": (c_int, [c_void_p] + [c_float] * 8),
    "mi_adsr_bank_create": (c_int, [POINTER(c_void_p), c_uint32]),
    "mi_adsr_bank_destroy": (c_int, [c_void_p]),
    "mi_adsr_bank_set": (c_int, [c_void_p, c_uint32, c_uint32, c_double, c_double, c_double]),
    "mi_adsr_bank_set_attack_time": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_adsr_bank_set_hold_time": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_adsr_bank_set_decay_time": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_adsr_bank_set_slope_time": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_adsr_bank_set_release_time": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_adsr_bank_set_attack_curve": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_adsr_bank_set_decay_curve": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_adsr_bank_set_slope_curve": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_adsr_bank_set_release_curve": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_adsr_bank_set_break_level": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_adsr_bank_set_sustain_level": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_adsr_bank_set_attack_function": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_adsr_bank_set_decay_function": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_adsr_bank_set_slope_function": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_adsr_bank_set_release_function": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_adsr_bank_set_hold_enabled": (c_int, [c_void_p, c_uint32, c_int]),
    "mi_adsr_bank_set_break_enabled": (c_int, [c_void_p, c_uint32, c_int]),
    "mi_adsr_bank_set_attack": (c_int, [c_void_p, c_uint32, c_float, c_float, c_uint32]),
    "mi_adsr_bank_set_decay": (c_int, [c_void_p, c_uint32, c_float, c_float, c_uint32]),
    "mi_adsr_bank_set_slope": (c_int, [c_void_p, c_uint32, c_float, c_float, c_uint32]),
    "mi_adsr_bank_set_release": (c_int, [c_void_p, c_uint32, c_float, c_float, c_uint32]),
    "mi_adsr_bank_set_hold": (c_int, [c_void_p, c_uint32, c_float, c_int]),
    "mi_adsr_bank_set_break": (c_int, [c_void_p, c_uint32, c_float, c_int]),
    "mi_adsr_bank_set_settings": (c_int, [c_void_p, c_uint32, POINTER(AdsrSettings)]),
    "mi_adsr_bank_get_settings": (c_int, [c_void_p, c_uint32, POINTER(AdsrSettings)]),
    "mi_adsr_bank_needs_update": (c_int, [c_void_p, c_uint32, POINTER(c_int)]),
    "mi_adsr_bank_update_settings": (c_int, [c_void_p, c_void_p]),
    "mi_adsr_bank_set_row_enabled": (c_int, [c_void_p, c_uint32, c_int]),
    "mi_adsr_bank_process": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_adsr_bank_process_mul": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_adsr_bank_generate": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_void_p]),
    "mi_adsr_bank_generate_mul": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_metergraph_bank_create": (c_int, [POINTER(c_void_p), c_uint32, c_uint32]),
    "mi_metergraph_bank_destroy": (c_int, [c_void_p]),
    "mi_metergraph_bank_init": (c_int, [c_void_p, c_uint32, c_size_t, c_size_t, c_float]),
    "mi_metergraph_bank_set_method": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_metergraph_bank_set_period": (c_int, [c_void_p, c_uint32, c_size_t]),
    "mi_metergraph_bank_set_default_value": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_metergraph_bank_fill": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_metergraph_bank_clear": (c_int, [c_void_p, c_uint32]),
    "mi_metergraph_bank_update_settings": (c_int, [c_void_p, c_void_p]),
    "mi_metergraph_bank_get_params": (c_int, [c_void_p, c_uint32, POINTER(MeterGraphParams)]),
    "mi_metergraph_bank_get_state": (c_int, [c_void_p, c_uint32, POINTER(MeterGraphState), c_void_p, c_void_p]),
    "mi_metergraph_bank_set_state": (c_int, [c_void_p, c_uint32, POINTER(MeterGraphState), c_void_p, c_void_p]),
    "mi_metergraph_bank_process": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_void_p]),
    "mi_metergraph_bank_process_value": (c_int, [c_void_p, c_void_p, c_void_p]),
    "mi_metergraph_bank_read": (c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p]),
    "mi_metergraph_bank_level": (c_int, [c_void_p, c_void_p, c_void_p]),
    "mi_scaled_metergraph_bank_create": (c_int, [POINTER(c_void_p), c_uint32, c_uint32, c_uint32]),
    "mi_scaled_metergraph_bank_destroy": (c_int, [c_void_p]),
    "mi_scaled_metergraph_bank_init": (c_int, [c_void_p, c_uint32, c_size_t, c_size_t, c_size_t]),
    "mi_scaled_metergraph_bank_set_method": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_scaled_metergraph_bank_set_period": (c_int, [c_void_p, c_uint32, c_size_t]),
    "mi_scaled_metergraph_bank_fill": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_scaled_metergraph_bank_update_settings": (c_int, [c_void_p, c_void_p]),
    "mi_scaled_metergraph_bank_get_params": (c_int, [c_void_p, c_uint32, POINTER(ScaledMeterGraphParams)]),
    "mi_scaled_metergraph_bank_get_state": (c_int, [c_void_p, c_uint32, POINTER(ScaledMeterGraphState), c_void_p, c_void_p, c_void_p]),
    "mi_scaled_metergraph_bank_set_state": (c_int, [c_void_p, c_uint32, POINTER(ScaledMeterGraphState), c_void_p, c_void_p, c_void_p]),
    "mi_scaled_metergraph_bank_process": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_void_p]),
    "mi_scaled_metergraph_bank_process_value": (c_int, [c_void_p, c_void_p, c_void_p]),
    "mi_scaled_metergraph_bank_read": (c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p]),
    "mi_scaled_metergraph_bank_level": (c_int, [c_void_p, c_void_p, c_void_p]),
    "mi_qcounter_bank_create": (c_int, [POINTER(c_void_p), c_uint32, c_size_t, c_size_t]),
    "mi_qcounter_bank_destroy": (c_int, [c_void_p]),
    "mi_qcounter_bank_set_period": (c_int, [c_void_p, c_uint32, c_size_t]),
    "mi_qcounter_bank_set_levels": (c_int, [c_void_p, c_uint32, c_size_t]),
    "mi_qcounter_bank_set_min_value": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_qcounter_bank_set_max_value": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_qcounter_bank_set_value_range": (c_int, [c_void_p, c_uint32, c_float, c_float]),
    "mi_qcounter_bank_set_range": (c_int, [c_void_p, c_uint32, c_float, c_float, c_size_t]),
    "mi_qcounter_bank_needs_update": (c_int, [c_void_p, c_uint32, POINTER(c_int)]),
    "mi_qcounter_bank_update_settings": (c_int, [c_void_p, c_void_p]),
    "mi_qcounter_bank_clear": (c_int, [c_void_p, c_uint32]),
    "mi_qcounter_bank_process": (c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p]),
    "mi_qcounter_bank_read": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "mi_qcounter_bank_get_params": (c_int, [c_void_p, c_uint32, POINTER(QuantizedCounterParams)]),
    "mi_qcounter_bank_get_state": (c_int, [c_void_p, c_uint32, POINTER(QuantizedCounterState), c_void_p, c_void_p, c_void_p]),
    "mi_qcounter_bank_set_state": (c_int, [c_void_p, c_uint32, POINTER(QuantizedCounterState), c_void_p, c_void_p, c_void_p]),
    "mi_qcounter_bank_set_wave_combining": (c_int, [c_void_p, c_int]),
    "mi_oscillator_settings_init": (c_int, [POINTER(OscillatorSettings)]),
    "mi_oscillator_settings_set": (c_int, [POINTER(OscillatorSettings), c_uint32, c_double, c_double]),
    "mi_oscillator_settings_update": (c_int, [POINTER(OscillatorSettings)]),
    "mi_oscillator_bank_create": (c_int, [POINTER(c_void_p), c_uint32]),
    "mi_oscillator_bank_destroy": (c_int, [c_void_p]),
    "mi_oscillator_bank_set": (c_int, [c_void_p, c_uint32, c_uint32, c_double, c_double]),
    "mi_oscillator_bank_set_function": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_oscillator_bank_set_frequency": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_oscillator_bank_set_sample_rate": (c_int, [c_void_p, c_uint32, c_size_t]),
    "mi_oscillator_bank_set_phase": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_oscillator_bank_set_phase_accumulator_bits": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_oscillator_bank_set_dc_offset": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_oscillator_bank_set_dc_reference": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_oscillator_bank_set_amplitude": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_oscillator_bank_set_duty_ratio": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_oscillator_bank_set_width": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_oscillator_bank_set_trapezoid_ratios": (c_int, [c_void_p, c_uint32, c_float, c_float]),
    "mi_oscillator_bank_set_pulsetrain_ratios": (c_int, [c_void_p, c_uint32, c_float, c_float]),
    "mi_oscillator_bank_set_parabolic_width": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_oscillator_bank_set_squared_sinusoid_inversion": (c_int, [c_void_p, c_uint32, c_int]),
    "mi_oscillator_bank_set_parabolic_inversion": (c_int, [c_void_p, c_uint32, c_int]),
    "mi_oscillator_bank_set_oversampler_mode": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_oscillator_bank_reset_phase_accumulator": (c_int, [c_void_p, c_uint32]),
    "mi_oscillator_bank_needs_update": (c_int, [c_void_p, c_uint32, POINTER(c_int)]),
    "mi_oscillator_bank_update_settings": (c_int, [c_void_p, c_void_p]),
    "mi_oscillator_bank_get_settings": (c_int, [c_void_p, c_uint32, POINTER(OscillatorSettings)]),
    "mi_oscillator_bank_set_settings": (c_int, [c_void_p, c_uint32, POINTER(OscillatorSettings)]),
    "mi_oscillator_bank_get_exact_frequency": (c_int, [c_void_p, c_uint32, POINTER(c_float)]),
    "mi_oscillator_bank_get_exact_phase": (c_int, [c_void_p, c_uint32, POINTER(c_float)]),
    "mi_oscillator_bank_process": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_uint32, c_void_p]),
    "mi_oscillator_bank_reserve": (c_int, [c_void_p, c_size_t]),
    "mi_oscillator_bank_set_exact": (c_int, [c_void_p, c_int]),
    "mi_oscillator_bank_get_state": (c_int, [c_void_p, c_uint32, POINTER(OscillatorState), c_void_p]),
    "mi_oscillator_bank_set_state": (c_int, [c_void_p, c_uint32, POINTER(OscillatorState), c_void_p]),
    "mi_oscillator_bank_get_periods": (c_int, [c_void_p, c_uint32, c_void_p, c_size_t, c_size_t, c_size_t, c_void_p]),
    "mi_oscillator_bank_synth_rows": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_size_t)]),
    "mi_velvet_bank_create": (c_int, [POINTER(c_void_p), c_uint32]),
    "mi_velvet_bank_destroy": (c_int, [c_void_p]),
    "mi_velvet_bank_init": (c_int, [c_void_p, c_uint32, c_uint32, c_uint32, c_uint64]),
    "mi_velvet_bank_init_time": (c_int, [c_void_p, c_uint32]),
    "mi_velvet_bank_set_core_type": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_velvet_bank_set_velvet_type": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_velvet_bank_set_velvet_window_width": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_velvet_bank_set_delta_value": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_velvet_bank_set_crush_probability": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_velvet_bank_set_amplitude": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_velvet_bank_set_offset": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_velvet_bank_set_crush": (c_int, [c_void_p, c_uint32, c_int]),
    "mi_velvet_bank_process": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_uint32, c_void_p]),
    "mi_velvet_bank_reserve": (c_int, [c_void_p, c_size_t]),
    "mi_velvet_bank_get_state": (c_int, [c_void_p, c_uint32, POINTER(VelvetState), c_void_p]),
    "mi_velvet_bank_set_state": (c_int, [c_void_p, c_uint32, POINTER(VelvetState), c_void_p]),
    "mi_velvet_bank_set_row_enabled": (c_int, [c_void_p, c_uint32, c_int]),
    "mi_velvet_bank_commit": (c_int, [c_void_p, c_void_p]),
    "mi_velvet_bank_process_segmented": (c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p]),
    "mi_lcg_seed_words": (c_int, [c_uint32, POINTER(LcgState)]),
    "mi_lcg_bank_create": (c_int, [POINTER(c_void_p), c_uint32]),
    "mi_lcg_bank_destroy": (c_int, [c_void_p]),
    "mi_lcg_bank_init": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_lcg_bank_init_time": (c_int, [c_void_p, c_uint32]),
    "mi_lcg_bank_set_distribution": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_lcg_bank_set_amplitude": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_lcg_bank_set_offset": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_lcg_bank_process": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_uint32, c_void_p]),
    "mi_lcg_bank_get_state": (c_int, [c_void_p, c_uint32, POINTER(LcgState), c_void_p]),
    "mi_lcg_bank_set_state": (c_int, [c_void_p, c_uint32, POINTER(LcgState), c_void_p]),
    "mi_lcg_bank_set_row_enabled": (c_int, [c_void_p, c_uint32, c_int]),
    "mi_lcg_bank_commit": (c_int, [c_void_p, c_void_p]),
    "mi_mls_settings_init": (c_int, [POINTER(MlsSettings)]),
    "mi_mls_settings_update": (c_int, [POINTER(MlsSettings)]),
    "mi_mls_tables": (c_int, [c_uint32, POINTER(c_uint64), POINTER(c_uint64)]),
    "mi_mls_advance": (c_int, [c_uint32, c_uint64, c_uint64, POINTER(c_uint64)]),
    "mi_mls_bank_create": (c_int, [POINTER(c_void_p), c_uint32]),
    "mi_mls_bank_destroy": (c_int, [c_void_p]),
    "mi_mls_bank_set_n_bits": (c_int, [c_void_p, c_uint32, c_size_t]),
    "mi_mls_bank_set_state": (c_int, [c_void_p, c_uint32, c_uint64]),
    "mi_mls_bank_set_amplitude": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_mls_bank_set_offset": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_mls_bank_needs_update": (c_int, [c_void_p, c_uint32, POINTER(c_int)]),
    "mi_mls_bank_update_settings": (c_int, [c_void_p, c_void_p]),
    "mi_mls_bank_maximum_number_of_bits": (c_int, [c_void_p, POINTER(c_size_t)]),
    "mi_mls_bank_get_period": (c_int, [c_void_p, c_uint32, POINTER(c_uint64)]),
    "mi_mls_bank_process": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_uint32, c_void_p]),
    "mi_mls_bank_reserve": (c_int, [c_void_p, c_size_t]),
    "mi_mls_bank_get_settings": (c_int, [c_void_p, c_uint32, POINTER(MlsSettings)]),
    "mi_mls_bank_get_state": (c_int, [c_void_p, c_uint32, POINTER(c_uint64), c_void_p]),
    "mi_mls_bank_set_row_enabled": (c_int, [c_void_p, c_uint32, c_int]),
    "mi_mls_bank_commit": (c_int, [c_void_p, c_void_p]),
    "mi_spectral_tilt_settings_init": (c_int, [POINTER(SpectralTiltSettings)]),
    "mi_spectral_tilt_settings_set_order": (c_int, [POINTER(SpectralTiltSettings), c_uint64]),
    "mi_spectral_tilt_settings_set_slope": (c_int, [POINTER(SpectralTiltSettings), c_float, c_uint32]),
    "mi_spectral_tilt_settings_set_norm": (c_int, [POINTER(SpectralTiltSettings), c_uint32]),
    "mi_spectral_tilt_settings_set_lower_frequency": (c_int, [POINTER(SpectralTiltSettings), c_float]),
    "mi_spectral_tilt_settings_set_upper_frequency": (c_int, [POINTER(SpectralTiltSettings), c_float]),
    "mi_spectral_tilt_settings_set_frequency_range": (c_int, [POINTER(SpectralTiltSettings), c_float, c_float]),
    "mi_spectral_tilt_settings_set_sample_rate": (c_int, [POINTER(SpectralTiltSettings), c_uint64]),
    "mi_spectral_tilt_settings_update": (c_int, [POINTER(SpectralTiltSettings), POINTER(c_int)]),
    "mi_spectral_tilt_settings_freq_chart": (c_int, [POINTER(SpectralTiltSettings), c_void_p, c_void_p, c_void_p, c_void_p, c_size_t]),
    "mi_spectral_tilt_settings_section_gain": (c_int, [POINTER(SpectralTiltSettings), POINTER(BiquadX1), c_float, POINTER(c_float)]),
    "mi_spectral_tilt_settings_normalise_section": (c_int, [POINTER(SpectralTiltSettings), POINTER(BiquadX1)]),
    "mi_spectral_tilt_bank_create": (c_int, [POINTER(c_void_p), c_uint32]),
    "mi_spectral_tilt_bank_destroy": (c_int, [c_void_p]),
    "mi_spectral_tilt_bank_set_order": (c_int, [c_void_p, c_uint32, c_size_t]),
    "mi_spectral_tilt_bank_set_slope": (c_int, [c_void_p, c_uint32, c_float, c_uint32]),
    "mi_spectral_tilt_bank_set_norm": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_spectral_tilt_bank_set_lower_frequency": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_spectral_tilt_bank_set_upper_frequency": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_spectral_tilt_bank_set_frequency_range": (c_int, [c_void_p, c_uint32, c_float, c_float]),
    "mi_spectral_tilt_bank_set_sample_rate": (c_int, [c_void_p, c_uint32, c_size_t]),
    "mi_spectral_tilt_bank_set_row_enabled": (c_int, [c_void_p, c_uint32, c_int]),
    "mi_spectral_tilt_bank_set_exact": (c_int, [c_void_p, c_int]),
    "mi_spectral_tilt_bank_update_settings": (c_int, [c_void_p, c_void_p]),
    "mi_spectral_tilt_bank_commit": (c_int, [c_void_p, c_void_p]),
    "mi_spectral_tilt_bank_reserve": (c_int, [c_void_p, c_size_t, c_void_p]),
    "mi_spectral_tilt_bank_process": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_uint32, c_void_p]),
    "mi_spectral_tilt_bank_get_chains": (c_int, [c_void_p, c_uint32, POINTER(BiquadX1), POINTER(c_uint32)]),
    "mi_spectral_tilt_bank_get_settings": (c_int, [c_void_p, c_uint32, POINTER(SpectralTiltSettings)]),
    "mi_spectral_tilt_bank_freq_chart": (c_int, [c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_size_t]),
    "mi_spectral_tilt_bank_freq_chart_packed": (c_int, [c_void_p, c_uint32, c_void_p, c_void_p, c_size_t]),
    "mi_spectral_tilt_bank_reset": (c_int, [c_void_p, c_uint32, c_void_p]),
    "mi_spectral_tilt_bank_get_state": (c_int, [c_void_p, c_uint32, c_void_p, c_void_p]),
    "mi_spectral_tilt_bank_set_state": (c_int, [c_void_p, c_uint32, c_void_p, c_void_p]),
    "mi_noise_generator_bank_create": (c_int, [POINTER(c_void_p), c_uint32]),
    "mi_noise_generator_bank_destroy": (c_int, [c_void_p]),
    "mi_noise_generator_bank_init": (c_int, [c_void_p, c_uint32, c_uint32, c_uint64, c_uint32, c_uint32, c_uint32, c_uint64]),
    "mi_noise_generator_bank_init_auto": (c_int, [c_void_p, c_uint32]),
    "mi_noise_generator_bank_set_sample_rate": (c_int, [c_void_p, c_uint32, c_size_t]),
    "mi_noise_generator_bank_set_mls_n_bits": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_noise_generator_bank_set_mls_seed": (c_int, [c_void_p, c_uint32, c_uint64]),
    "mi_noise_generator_bank_set_lcg_distribution": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_noise_generator_bank_set_velvet_type": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_noise_generator_bank_set_velvet_window_width": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_noise_generator_bank_set_velvet_arn_delta": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_noise_generator_bank_set_velvet_crush": (c_int, [c_void_p, c_uint32, c_int]),
    "mi_noise_generator_bank_set_velvet_crushing_probability": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_noise_generator_bank_set_generator": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_noise_generator_bank_set_noise_color": (c_int, [c_void_p, c_uint32, c_uint32]),
    "mi_noise_generator_bank_set_coloring_order": (c_int, [c_void_p, c_uint32, c_size_t]),
    "mi_noise_generator_bank_set_color_slope": (c_int, [c_void_p, c_uint32, c_float, c_uint32]),
    "mi_noise_generator_bank_set_amplitude": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_noise_generator_bank_set_offset": (c_int, [c_void_p, c_uint32, c_float]),
    "mi_noise_generator_bank_set_exact": (c_int, [c_void_p, c_int]),
    "mi_noise_generator_bank_update_settings": (c_int, [c_void_p, c_void_p]),
    "mi_noise_generator_bank_reserve": (c_int, [c_void_p, c_size_t, c_void_p]),
    "mi_noise_generator_bank_process": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_uint32, c_void_p]),
    "mi_noise_generator_bank_freq_chart": (c_int, [c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_size_t]),
    "mi_noise_generator_bank_freq_chart_packed": (c_int, [c_void_p, c_uint32, c_void_p, c_void_p, c_size_t]),
    "mi_noise_generator_bank_get_settings": (c_int, [c_void_p, c_uint32, POINTER(NoiseGeneratorSettings)]),
    "mi_noise_generator_bank_get_tilt_settings": (c_int, [c_void_p, c_uint32, POINTER(SpectralTiltSettings)]),
    "mi_noise_generator_bank_get_state": (c_int, [c_void_p, c_uint32, POINTER(NoiseGeneratorState), c_void_p]),
    "mi_noise_generator_bank_set_state": (c_int, [c_void_p, c_uint32, POINTER(NoiseGeneratorState), c_void_p]),
    "mi_delay_bank_create": (c_int, [POINTER(c_void_p), c_uint32, c_size_t]),
    "mi_delay_bank_destroy": (c_int, [c_void_p]),
    "mi_delay_bank_set_delay": (c_int, [c_void_p, c_uint32, c_size_t]),
    "mi_delay_bank_get": (c_int, [c_void_p, c_uint32, POINTER(c_uint32), POINTER(c_uint32), POINTER(c_uint32), POINTER(c_uint32)]),
    "mi_delay_bank_clear": (c_int, [c_void_p, c_void_p]),
    "mi_delay_bank_append": (c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p]),
    "mi_delay_bank_process": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_int, c_int, c_float,
                                      c_void_p, c_size_t, c_void_p]),
    "mi_delay_bank_append_rows": (c_int, [c_void_p, c_void_p, c_uint32, c_void_p, c_size_t, c_size_t, c_void_p]),
    "mi_delay_bank_process_rows": (c_int, [c_void_p, c_void_p, c_uint32, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_int, c_int,
                                   c_float, c_void_p, c_size_t, c_void_p]),
    "mi_delay_bank_process_ramping": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_int,
                                              c_float, c_void_p, c_size_t, c_void_p]),
    "mi_delay_bank_process_ramping_rows": (c_int, [c_void_p, c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_int,
                                              c_float, c_void_p, c_size_t, c_void_p]),
    "mi_ring_bank_create": (c_int, [POINTER(c_void_p), c_uint32, c_size_t, c_float]),
    "mi_ring_bank_create_shared": (c_int, [POINTER(c_void_p), c_uint32, c_size_t, c_float, POINTER(c_void_p)]),
    "mi_ring_bank_destroy": (c_int, [c_void_p]),
    "mi_ring_bank_fill": (c_int, [c_void_p, c_float, c_void_p]),
    "mi_ring_bank_append": (c_int, [c_void_p, c_void_p, c_size_t, c_size_t, POINTER(c_size_t), c_void_p]),
    "mi_ring_bank_get": (c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, POINTER(c_size_t), c_void_p]),
    "mi_ring_bank_info": (c_int, [c_void_p, c_size_t, POINTER(c_uint32), POINTER(c_uint32), POINTER(c_uint32)]),
    "mi_biquad_section_tables": (c_int, [POINTER(BiquadX1), c_int, POINTER(c_float), POINTER(c_uint32)]),
}

for _name, (_res, _args) in PROTOTYPES.items():
    _fn = getattr(lib, _name)          # AttributeError here == symbol missing from the .so
    _fn.restype = _res
    _fn.argtypes = _args


def check(code):
    if code != 0:
        raise MiError(code, (lib.mi_dspu_last_error() or b"").decode("utf-8", "replace"))
    return code


SPECTRAL_FUNC = ctypes.CFUNCTYPE(None, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_void_p)
SPLITTER_FUNC = ctypes.CFUNCTYPE(None, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_void_p)
OVERSAMPLER_FUNC = ctypes.CFUNCTYPE(c_int, c_void_p, c_size_t, c_size_t, c_uint32, c_void_p, c_void_p)
