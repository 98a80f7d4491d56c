"""Small object wrappers over the C-ABI handles (no arithmetic here)."""
import ctypes
from ctypes import byref, c_float, c_int, c_uint32, c_void_p

import numpy as np

from .capi import BiquadX1, FilterCascade, FilterParams, check, lib


def device_count():
    return int(lib.mi_dspu_device_count())


def last_launch():
    """The hot-path kernel this thread launched last (mi_dspu_last_launch): which launch a call took."""
    return (lib.mi_dspu_last_launch() or b"").decode()


def source_sha(name):
    """SHA-256 (16 hex digits) of csrc/<name> as the loaded library was built from it (mi_dspu_source_sha), or None."""
    v = lib.mi_dspu_source_sha(name.encode())
    return v.decode() if v else None


def last_stream_clock():
    """(GHz, microseconds) of the last mi_biquad_bank_process_blocks launch (mi_dspu_last_stream_clock)."""
    g, us = ctypes.c_double(), ctypes.c_double()
    check(lib.mi_dspu_last_stream_clock(byref(g), byref(us)))
    return g.value, us.value


def _ptr(x):
    """Device address of a DeviceBuffer, a torch tensor or a raw int."""
    if isinstance(x, DeviceBuffer):
        return c_void_p(x.ptr)
    if hasattr(x, "data_ptr"):
        return c_void_p(x.data_ptr())
    return c_void_p(int(x))


def _stream(s):
    if s is None:
        return c_void_p(0)
    if hasattr(s, "cuda_stream"):
        return c_void_p(s.cuda_stream)
    return c_void_p(int(s))


class DeviceBuffer:
    """float32 device array owned by the library allocator (mi_dspu_malloc)."""

    def __init__(self, shape):
        self.shape = tuple(int(v) for v in (shape if hasattr(shape, "__len__") else (shape,)))
        self.size = int(np.prod(self.shape)) if self.shape else 1
        p = c_void_p()
        check(lib.mi_dspu_malloc(byref(p), self.size * 4))
        self.ptr = p.value or 0

    @classmethod
    def from_host(cls, array, stream=None):
        a = np.ascontiguousarray(array, dtype=np.float32)
        buf = cls(a.shape)
        buf.upload(a, stream)
        return buf

    def upload(self, array, stream=None):
        a = np.ascontiguousarray(array, dtype=np.float32)
        assert a.size == self.size
        check(lib.mi_dspu_copy_h2d(c_void_p(self.ptr), a.ctypes.data_as(c_void_p), a.nbytes, _stream(stream)))
        check(lib.mi_dspu_stream_synchronize(_stream(stream)))

    def download(self, stream=None):
        out = np.empty(self.shape, dtype=np.float32)
        check(lib.mi_dspu_copy_d2h(out.ctypes.data_as(c_void_p), c_void_p(self.ptr), out.nbytes, _stream(stream)))
        check(lib.mi_dspu_stream_synchronize(_stream(stream)))
        return out

    def zero(self, stream=None):
        check(lib.mi_dspu_memset(c_void_p(self.ptr), 0, self.size * 4, _stream(stream)))

    def free(self):
        if self.ptr:
            lib.mi_dspu_free(c_void_p(self.ptr))
            self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _chains(coefs):
    """(n,5) float32 {b0,b1,b2,a1,a2} rows -> ctypes array of mi_biquad_x1_t."""
    c = np.ascontiguousarray(coefs, dtype=np.float32).reshape(-1, 5)
    full = np.zeros((c.shape[0], 8), dtype=np.float32)
    full[:, :5] = c
    arr = (BiquadX1 * max(1, c.shape[0])).from_buffer_copy(full.tobytes() if c.shape[0] else bytes(32))
    return arr, c.shape[0]


class BiquadBank:
    """`channels` x lsp::dspu::FilterBank on the device (mi_biquad_bank_*)."""

    def __init__(self, channels, max_sections):
        h = c_void_p()
        check(lib.mi_biquad_bank_create(byref(h), channels, max_sections))
        self.handle = h
        self.channels = channels
        self.max_sections = max(1, max_sections)

    def set_chains(self, channel, coefs, clear=False):
        arr, n = _chains(coefs)
        check(lib.mi_biquad_bank_set_chains(self.handle, channel, arr, n, int(clear)))

    def set_row_enabled(self, channel, enabled=True):
        """A channel that is switched off is skipped by process(): state kept, output row not written."""
        check(lib.mi_biquad_bank_set_row_enabled(self.handle, channel, 1 if enabled else 0))

    def set_exact(self, on=True):
        """The reference's serial recurrence, bit for bit (mi_biquad_bank_set_exact), instead of the time-parallel kernels."""
        check(lib.mi_biquad_bank_set_exact(self.handle, 1 if on else 0))

    def set_all_chains(self, coefs, clear=False):
        c = np.ascontiguousarray(coefs, dtype=np.float32)
        assert c.ndim == 3 and c.shape[0] == self.channels and c.shape[2] == 5
        arr, _ = _chains(c.reshape(-1, 5))
        check(lib.mi_biquad_bank_set_all_chains(self.handle, arr, c.shape[1], int(clear)))

    def size(self, channel):
        n = c_uint32()
        check(lib.mi_biquad_bank_size(self.handle, channel, byref(n)))
        return n.value

    def commit(self, stream=None):
        check(lib.mi_biquad_bank_commit(self.handle, _stream(stream)))

    def reset(self, channel=None, stream=None):
        check(lib.mi_biquad_bank_reset(self.handle, 0xFFFFFFFF if channel is None else channel, _stream(stream)))

    def process(self, out, inp, samples, out_stride=None, in_stride=None, stream=None):
        check(lib.mi_biquad_bank_process(self.handle, _ptr(out), _ptr(inp), samples,
                                         samples if out_stride is None else out_stride,
                                         samples if in_stride is None else in_stride, _stream(stream)))

    def process_blocks(self, outs, inps, samples, out_stride=None, in_stride=None, stream=None):
        """len(outs) consecutive process() calls issued by one C call (mi_biquad_bank_process_blocks)."""
        n = len(outs)
        assert n == len(inps)
        po = (c_void_p * n)(*[_ptr(b) for b in outs])
        pi = (c_void_p * n)(*[_ptr(b) for b in inps])
        check(lib.mi_biquad_bank_process_blocks(self.handle, po, pi, n, samples,
                                                samples if out_stride is None else out_stride,
                                                samples if in_stride is None else in_stride, _stream(stream)))

    def impulse_response(self, out, samples, out_stride=None, stream=None):
        check(lib.mi_biquad_bank_impulse_response(self.handle, _ptr(out), samples,
                                                  samples if out_stride is None else out_stride, _stream(stream)))

    def get_state(self, stream=None):
        st = np.empty((self.channels, self.max_sections, 2), dtype=np.float32)
        check(lib.mi_biquad_bank_get_state(self.handle, st.ctypes.data_as(c_void_p), _stream(stream)))
        return st

    def set_state(self, state, stream=None):
        st = np.ascontiguousarray(state, dtype=np.float32)
        assert st.shape == (self.channels, self.max_sections, 2)
        check(lib.mi_biquad_bank_set_state(self.handle, st.ctypes.data_as(c_void_p), _stream(stream)))

    def close(self):
        if self.handle:
            lib.mi_biquad_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ConvolverBank:
    """`channels` x lsp::dspu::Convolver on the device (mi_convolver_bank_*)."""

    def __init__(self, irs, rank, counts=None, phase=0.0, stream=None):
        irs = np.ascontiguousarray(irs, dtype=np.float32)
        if irs.ndim == 1:
            irs = irs.reshape(1, -1)
        self.channels = irs.shape[0]
        cnt = None
        if counts is not None:
            cnt = np.ascontiguousarray(counts, dtype=np.uint32)
            assert cnt.shape == (self.channels,)
        h = c_void_p()
        check(lib.mi_convolver_bank_create(byref(h), self.channels,
                                           irs.ctypes.data_as(c_void_p) if irs.size else None, irs.shape[1],
                                           cnt.ctypes.data_as(c_void_p) if cnt is not None else None,
                                           irs.shape[1], rank, phase, _stream(stream)))
        self.handle = h

    def info(self):
        v = [c_uint32() for _ in range(4)]
        check(lib.mi_convolver_bank_info(self.handle, *[byref(x) for x in v]))
        return dict(zip(("rank", "frame", "partitions", "data_size"), [x.value for x in v]))

    def faults(self, stream=None):
        """How often the two roles of the one-launch frame step gave up waiting for each other (0 on a healthy device)."""
        n = c_uint32(0)
        check(lib.mi_convolver_bank_faults(self.handle, byref(n), _stream(stream)))
        return int(n.value)

    def reset(self, stream=None):
        check(lib.mi_convolver_bank_reset(self.handle, _stream(stream)))

    def process(self, out, inp, samples, out_stride=None, in_stride=None, stream=None):
        check(lib.mi_convolver_bank_process(self.handle, _ptr(out), _ptr(inp), samples,
                                            samples if out_stride is None else out_stride,
                                            samples if in_stride is None else in_stride, _stream(stream)))

    def process_blocks(self, outs, inps, samples, out_stride=None, in_stride=None, stream=None):
        """len(outs) consecutive process() calls issued by one C call (mi_convolver_bank_process_blocks)."""
        n = len(outs)
        assert n == len(inps)
        po = (c_void_p * n)(*[_ptr(b) for b in outs])
        pi = (c_void_p * n)(*[_ptr(b) for b in inps])
        check(lib.mi_convolver_bank_process_blocks(self.handle, po, pi, n, samples,
                                                   samples if out_stride is None else out_stride,
                                                   samples if in_stride is None else in_stride, _stream(stream)))

    def close(self):
        if self.handle:
            lib.mi_convolver_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def design_filter(ftype, slope=1, freq=1000.0, freq2=1000.0, gain=1.0, quality=0.0, sample_rate=48000):
    """Filter::update + rebuild on the host: returns (mode, cascades[n][2][3], sections[n][5])."""
    fp = FilterParams(int(ftype), int(slope), float(freq), float(freq2), float(gain), float(quality))
    chains = (BiquadX1 * 256)()
    casc = (FilterCascade * 256)()
    nch, nca, mode = c_uint32(), c_uint32(), ctypes.c_int()
    check(lib.mi_filter_design(byref(fp), sample_rate, chains, 256, byref(nch), casc, 256, byref(nca), byref(mode)))
    sec = np.array([[c.b0, c.b1, c.b2, c.a1, c.a2] for c in chains[:nch.value]], dtype=np.float32).reshape(-1, 5)
    cas = np.array([[list(c.t)[:3], list(c.b)[:3]] for c in casc[:nca.value]], dtype=np.float32).reshape(-1, 2, 3)
    return mode.value, cas, sec


def filter_freq_chart(freqs, ftype, slope=1, freq=1000.0, freq2=1000.0, gain=1.0, quality=0.0, sample_rate=48000):
    fp = FilterParams(int(ftype), int(slope), float(freq), float(freq2), float(gain), float(quality))
    f = np.ascontiguousarray(freqs, dtype=np.float32)
    c = np.empty(2 * f.size, np.float32)
    check(lib.mi_filter_freq_chart(byref(fp), sample_rate, c.ctypes.data_as(c_void_p), f.ctypes.data_as(c_void_p), f.size))
    return c[0::2] + 1j * c[1::2]


def make_window(n, wtype):
    out = np.empty(n, np.float32)
    check(lib.mi_window(out.ctypes.data_as(c_void_p), n, int(wtype)))
    return out


def make_window_general(n, wtype, params):
    """windows::*_general (misc/windows.h:71-155): the window family `wtype` with its parameter list."""
    out = np.empty(n, np.float32)
    q = np.ascontiguousarray(params, dtype=np.float32)
    check(lib.mi_window_general(out.ctypes.data_as(c_void_p), n, int(wtype), q.ctypes.data_as(c_void_p), q.size))
    return out


class SpectralBank:
    """`channels` x lsp::dspu::SpectralProcessor (one MultiSpectralProcessor) on the device."""
    OP_NONE, OP_MASK, OP_CALLBACK = 0, 1, 2

    def __init__(self, channels, max_rank):
        h = c_void_p()
        check(lib.mi_spectral_bank_create(byref(h), channels, max_rank))
        self.handle, self.channels = h, channels
        self._cb = None

    def set_rank(self, rank):
        check(lib.mi_spectral_bank_set_rank(self.handle, rank))

    def set_phase(self, phase):
        check(lib.mi_spectral_bank_set_phase(self.handle, phase))

    def set_timing(self, eager):
        """False: SpectralProcessor (a full frame is transformed when the next sample arrives); True: Multi..."""
        check(lib.mi_spectral_bank_set_timing(self.handle, 1 if eager else 0))

    def get(self):
        v = [c_uint32() for _ in range(3)]
        check(lib.mi_spectral_bank_get(self.handle, *[byref(x) for x in v]))
        return dict(zip(("rank", "latency", "remaining"), [x.value for x in v]))

    def bind(self, pyfunc):
        """pyfunc(spectrum_dev_ptr, rank, channels, stream) runs on the host between the two transforms."""
        from .capi import SPECTRAL_FUNC
        if pyfunc is None:
            check(lib.mi_spectral_bank_unbind(self.handle))
            self._cb = None
            return
        self._cb = SPECTRAL_FUNC(lambda obj, subj, spec, rank, ch, st: pyfunc(spec, rank, ch, st))
        check(lib.mi_spectral_bank_bind(self.handle, ctypes.cast(self._cb, c_void_p), None, None))

    def bind_mask(self, mask, stream=None):
        m = np.ascontiguousarray(mask, dtype=np.float32)
        stride = 0 if m.ndim == 1 else m.shape[1]
        check(lib.mi_spectral_bank_bind_mask(self.handle, m.ctypes.data_as(c_void_p), stride, _stream(stream)))

    def bind_channels(self, has_in=None, has_out=None, stream=None):
        a = None if has_in is None else np.ascontiguousarray(has_in, dtype=np.uint8)
        b = None if has_out is None else np.ascontiguousarray(has_out, dtype=np.uint8)
        check(lib.mi_spectral_bank_bind_channels(self.handle, a.ctypes.data_as(c_void_p) if a is not None else None,
                                                 b.ctypes.data_as(c_void_p) if b is not None else None, _stream(stream)))

    def reset(self, stream=None):
        check(lib.mi_spectral_bank_reset(self.handle, _stream(stream)))

    def process(self, out, inp, count, out_stride=None, in_stride=None, stream=None):
        check(lib.mi_spectral_bank_process(self.handle, _ptr(out) if out is not None else None, _ptr(inp), count,
                                           count if out_stride is None else out_stride,
                                           count if in_stride is None else in_stride, _stream(stream)))

    def process_blocks(self, outs, inps, count, out_stride=None, in_stride=None, stream=None):
        """len(outs) consecutive process() calls issued by one C call (mi_spectral_bank_process_blocks)."""
        n = len(outs)
        assert n == len(inps)
        po = (c_void_p * n)(*[(_ptr(b) if b is not None else None) for b in outs])
        pi = (c_void_p * n)(*[_ptr(b) for b in inps])
        check(lib.mi_spectral_bank_process_blocks(self.handle, po, pi, n, count,
                                                  count if out_stride is None else out_stride,
                                                  count if in_stride is None else in_stride, _stream(stream)))

    def close(self):
        if self.handle:
            lib.mi_spectral_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class AnalyzerBank:
    """lsp::dspu::Analyzer with `channels` channels on the device."""
    SAMPLE_RATE, RATE, WINDOW, ENVELOPE, SHIFT, REACTIVITY, RANK, ACTIVE = range(8)
    CH_FREEZE, CH_ENABLE, CH_DELAY = range(3)

    def __init__(self, channels, max_rank, max_sample_rate, min_rate, max_delay=0):
        h = c_void_p()
        check(lib.mi_analyzer_bank_create(byref(h), channels, max_rank, max_sample_rate, min_rate, max_delay))
        self.handle, self.channels = h, channels

    def configure(self, what, value):
        check(lib.mi_analyzer_bank_configure(self.handle, what, float(value)))

    def channel(self, channel, what, value):
        check(lib.mi_analyzer_bank_channel(self.handle, channel, what, int(value)))

    def process(self, inp, samples, in_stride=None, stream=None):
        check(lib.mi_analyzer_bank_process(self.handle, _ptr(inp) if inp is not None else None, samples,
                                           samples if in_stride is None else in_stride, _stream(stream)))

    def info(self):
        v = [c_uint32() for _ in range(4)]
        check(lib.mi_analyzer_bank_info(self.handle, *[byref(x) for x in v]))
        return dict(zip(("rank", "bins", "period", "step"), [x.value for x in v]))

    def get_spectrum(self, idx, stream=None):
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
        didx = c_void_p()
        check(lib.mi_dspu_malloc(byref(didx), idx.nbytes))
        check(lib.mi_dspu_copy_h2d(didx, idx.ctypes.data_as(c_void_p), idx.nbytes, _stream(stream)))
        out = DeviceBuffer((self.channels, idx.size))
        check(lib.mi_analyzer_bank_get_spectrum(self.handle, c_void_p(out.ptr), idx.size, didx, idx.size, _stream(stream)))
        res = out.download(stream)
        lib.mi_dspu_free(didx)
        return res

    def allreduce_bins(self, bins, frames, comm, stream=None):
        """Sum `bins` (device [frames][bins]) over the ranks of `comm` in place: RCCL from the library's host side."""
        check(lib.mi_analyzer_bank_allreduce_bins(self.handle, _ptr(bins), int(frames), comm.handle, _stream(stream)))

    def allreduce_bins_begin(self, partial, total, frames, comm, slot, stream=None):
        """The same collective on the communicator's side stream, behind what `stream` has enqueued so far; comm.wait(slot, stream)
        before `total` is read or the slot's buffers are written again (mi_analyzer_bank_allreduce_bins_begin)."""
        check(lib.mi_analyzer_bank_allreduce_bins_begin(self.handle, _ptr(partial), _ptr(total), int(frames), comm.handle, int(slot), _stream(stream)))

    def reduce_bins(self, out, with_envelope=False, stream=None):
        check(lib.mi_analyzer_bank_reduce_bins(self.handle, _ptr(out), int(with_envelope), _stream(stream)))

    def process_reduce(self, inp, samples, out, with_envelope=False, in_stride=None, stream=None):
        """process() + reduce_bins(), the reduction riding on the analysis launch (mi_analyzer_bank_process_reduce)."""
        check(lib.mi_analyzer_bank_process_reduce(self.handle, _ptr(inp) if inp is not None else None, samples,
                                                  samples if in_stride is None else in_stride, _ptr(out),
                                                  int(with_envelope), _stream(stream)))

    def process_reduce_frames(self, inps, samples, out, with_envelope=False, in_stride=None, out_stride=None, stream=None):
        """len(inps) consecutive process_reduce() calls in one C call; frame k's sums go to row k of `out`."""
        n = len(inps)
        pi = (c_void_p * n)(*[_ptr(b) for b in inps])
        bins = self.info()["bins"]
        check(lib.mi_analyzer_bank_process_reduce_frames(self.handle, pi, n, samples, samples if in_stride is None else in_stride,
                                                         _ptr(out), bins if out_stride is None else out_stride, int(with_envelope),
                                                         _stream(stream)))

    def close(self):
        if self.handle:
            lib.mi_analyzer_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def dynfilter_sections(ftype, slope, freq, freq2, quality, gain, sample_rate=48000):
    """Host: the digital sections of a dynamic filter at a fixed gain, (n, 5) float32."""
    fp = FilterParams(int(ftype), int(slope), float(freq), float(freq2), 1.0, float(quality))
    n = c_uint32()
    arr = (BiquadX1 * 128)()
    check(lib.mi_dynfilter_sections(byref(fp), int(sample_rate), float(gain), arr, 128, byref(n)))
    return np.array([[c.b0, c.b1, c.b2, c.a1, c.a2] for c in arr[:n.value]], dtype=np.float32).reshape(-1, 5)


def dynfilter_freq_chart(freqs, ftype, slope, freq, freq2, quality, gain, sample_rate=48000):
    fp = FilterParams(int(ftype), int(slope), float(freq), float(freq2), 1.0, float(quality))
    f = np.ascontiguousarray(freqs, dtype=np.float32)
    c = np.empty(2 * f.size, np.float32)
    check(lib.mi_dynfilter_freq_chart(byref(fp), int(sample_rate), c.ctypes.data_as(c_void_p), f.ctypes.data_as(c_void_p),
                                      float(gain), f.size))
    return c[0::2] + 1j * c[1::2]


class DynFilterBank:
    """`channels` x lsp::dspu::DynamicFilters(filters) on the device (shared settings, per-channel gain curves)."""

    def __init__(self, channels, filters):
        self.channels, self.filters = int(channels), int(filters)
        h = c_void_p()
        check(lib.mi_dynfilter_bank_create(byref(h), self.channels, self.filters))
        self.handle = h

    def set_sample_rate(self, sr):
        check(lib.mi_dynfilter_bank_set_sample_rate(self.handle, int(sr)))

    def set_params(self, fid, ftype, slope, freq, freq2, gain, quality):
        fp = FilterParams(int(ftype), int(slope), float(freq), float(freq2), float(gain), float(quality))
        check(lib.mi_dynfilter_bank_set_params(self.handle, int(fid), byref(fp)))

    def get_params(self, fid):
        fp, act = FilterParams(), c_int()
        check(lib.mi_dynfilter_bank_get_params(self.handle, int(fid), byref(fp), byref(act)))
        return dict(nType=fp.nType, nSlope=fp.nSlope, fFreq=fp.fFreq, fFreq2=fp.fFreq2, fGain=fp.fGain, fQuality=fp.fQuality), bool(act.value)

    def set_filter_active(self, fid, active=True):
        check(lib.mi_dynfilter_bank_set_filter_active(self.handle, int(fid), 1 if active else 0))

    def process(self, fid, out, inp, gain, samples, out_stride=None, in_stride=None, gain_stride=None, stream=None):
        check(lib.mi_dynfilter_bank_process(self.handle, int(fid), _ptr(out), _ptr(inp), _ptr(gain) if gain is not None else c_void_p(0),
                                            int(samples), int(out_stride or samples), int(in_stride or samples),
                                            int(gain_stride or samples), _stream(stream)))

    def close(self):
        if self.handle is not None:
            lib.mi_dynfilter_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Comm:
    """mi_dspu_comm_t: an RCCL communicator owned by the library (one process per GPU)."""

    ID_BYTES = 128

    @staticmethod
    def unique_id():
        buf = ctypes.create_string_buffer(Comm.ID_BYTES)
        check(lib.mi_dspu_comm_unique_id(buf))
        return bytes(buf.raw)

    def __init__(self, unique_id, nranks, rank):
        assert len(unique_id) == Comm.ID_BYTES
        h = c_void_p()
        check(lib.mi_dspu_comm_create(byref(h), ctypes.c_char_p(unique_id), int(nranks), int(rank)))
        self.handle = h

    def info(self):
        n, r = c_int(), c_int()
        check(lib.mi_dspu_comm_info(self.handle, byref(n), byref(r)))
        return n.value, r.value

    def wait(self, slot, stream=None):
        """`stream` waits (on the device) for the collective begun in `slot` (mi_dspu_comm_wait)."""
        check(lib.mi_dspu_comm_wait(self.handle, int(slot), _stream(stream)))

    def close(self):
        if self.handle is not None:
            lib.mi_dspu_comm_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DelayBank:
    """`channels` x lsp::dspu::Delay on the device."""

    def __init__(self, channels, max_size):
        h = c_void_p()
        check(lib.mi_delay_bank_create(byref(h), channels, max_size))
        self.handle, self.channels = h, channels

    def set_delay(self, delay, channel=None):
        check(lib.mi_delay_bank_set_delay(self.handle, 0xFFFFFFFF if channel is None else channel, int(delay)))

    def get(self, channel=0):
        v = [c_uint32() for _ in range(4)]
        check(lib.mi_delay_bank_get(self.handle, channel, *[byref(x) for x in v]))
        return dict(zip(("delay", "size", "head", "tail"), [x.value for x in v]))

    def clear(self, stream=None):
        check(lib.mi_delay_bank_clear(self.handle, _stream(stream)))

    def append(self, inp, count, in_stride=None, stream=None):
        check(lib.mi_delay_bank_append(self.handle, _ptr(inp), count, count if in_stride is None else in_stride, _stream(stream)))

    def process(self, out, inp, count, add=False, gain=None, gain_vec=None, out_stride=None, in_stride=None, stream=None):
        mode = 2 if gain_vec is not None else (1 if gain is not None else 0)
        check(lib.mi_delay_bank_process(self.handle, _ptr(out), _ptr(inp), count,
                                        count if out_stride is None else out_stride,
                                        count if in_stride is None else in_stride, int(add), mode,
                                        0.0 if gain is None else float(gain),
                                        _ptr(gain_vec) if gain_vec is not None else None, count, _stream(stream)))

    def append_rows(self, rows, inp, count, in_stride=None, stream=None):
        """Delay::append for the listed lines only (row r of `inp` belongs to channel rows[r])."""
        rw = np.ascontiguousarray(rows, dtype=np.uint32)
        check(lib.mi_delay_bank_append_rows(self.handle, rw.ctypes.data_as(c_void_p), len(rw), _ptr(inp), count,
                                            count if in_stride is None else in_stride, _stream(stream)))

    def process_rows(self, rows, out, inp, count, add=False, gain=None, gain_vec=None, out_stride=None, in_stride=None, stream=None):
        """Delay::process for the listed lines only: they alone are written and move on."""
        rw = np.ascontiguousarray(rows, dtype=np.uint32)
        mode = 2 if gain_vec is not None else (1 if gain is not None else 0)
        check(lib.mi_delay_bank_process_rows(self.handle, rw.ctypes.data_as(c_void_p), len(rw), _ptr(out), _ptr(inp), count,
                                             count if out_stride is None else out_stride,
                                             count if in_stride is None else in_stride, int(add), mode,
                                             0.0 if gain is None else float(gain),
                                             _ptr(gain_vec) if gain_vec is not None else None, count, _stream(stream)))

    def process_ramping(self, out, inp, new_delays, count, gain=None, gain_vec=None, stream=None):
        nd = np.ascontiguousarray(new_delays, dtype=np.uint32)
        assert nd.shape == (self.channels,)
        mode = 2 if gain_vec is not None else (1 if gain is not None else 0)
        check(lib.mi_delay_bank_process_ramping(self.handle, _ptr(out), _ptr(inp), nd.ctypes.data_as(c_void_p), count,
                                                count, count, mode, 0.0 if gain is None else float(gain),
                                                _ptr(gain_vec) if gain_vec is not None else None, count, _stream(stream)))

    def process_ramping_rows(self, rows, out, inp, new_delays, count, gain=None, gain_vec=None, stream=None):
        """Delay::process_ramping for the listed lines only (row r of the buffers and new_delays[r] belong to line rows[r])."""
        rw = np.ascontiguousarray(rows, dtype=np.uint32)
        nd = np.ascontiguousarray(new_delays, dtype=np.uint32)
        assert nd.shape == rw.shape
        mode = 2 if gain_vec is not None else (1 if gain is not None else 0)
        check(lib.mi_delay_bank_process_ramping_rows(self.handle, rw.ctypes.data_as(c_void_p), len(rw), _ptr(out), _ptr(inp),
                                                     nd.ctypes.data_as(c_void_p), count, count, count, mode,
                                                     0.0 if gain is None else float(gain),
                                                     _ptr(gain_vec) if gain_vec is not None else None, count, _stream(stream)))

    def close(self):
        if self.handle:
            lib.mi_delay_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DynamicDelayBank:
    """`channels` x lsp::dspu::DynamicDelay (mi_dyndelay_bank_*): delay, feedback gain and feedback delay per sample from three
    rows; the lines and nHead on the device."""

    def __init__(self, channels, max_size):
        h = c_void_p()
        check(lib.mi_dyndelay_bank_create(byref(h), channels, max_size))
        self.handle, self.channels = h, channels
        info = self.get(0, head=False)
        self.max_delay, self.capacity = info["max_delay"], info["capacity"]

    def get(self, channel=0, head=True):
        v = [c_uint32() for _ in range(3)]
        check(lib.mi_dyndelay_bank_get(self.handle, channel, byref(v[0]), byref(v[1]), byref(v[2]) if head else None))
        return dict(zip(("max_delay", "capacity", "head"), [x.value for x in v][:3 if head else 2]))

    def get_state(self, channel, stream=None):
        from .capi import DynDelayState
        s = DynDelayState()
        check(lib.mi_dyndelay_bank_get_state(self.handle, channel, byref(s), _stream(stream)))
        return {"head": s.head}

    def set_state(self, channel, head, stream=None):
        from .capi import DynDelayState
        s = DynDelayState(int(head))
        check(lib.mi_dyndelay_bank_set_state(self.handle, channel, byref(s), _stream(stream)))

    def clear(self, stream=None):
        check(lib.mi_dyndelay_bank_clear(self.handle, _stream(stream)))

    def process(self, out, inp, delay, fgain, fdelay, count, out_stride=None, in_stride=None, delay_stride=None, fgain_stride=None,
                fdelay_stride=None, stream=None):
        """process(out, in, delay, fgain, fdelay, count); out may be any of the four inputs (same stride)."""
        strides = [count if s is None else s for s in (out_stride, in_stride, delay_stride, fgain_stride, fdelay_stride)]
        check(lib.mi_dyndelay_bank_process(self.handle, _opt(out), _opt(inp), _opt(delay), _opt(fgain), _opt(fdelay), count, *strides,
                                           _stream(stream)))

    def copy(self, channel, src, src_channel, stream=None):
        """copy(s): line `channel` of this bank takes the newest samples of line `src_channel` of the bank `src`."""
        check(lib.mi_dyndelay_bank_copy(self.handle, channel, src.handle, src_channel, _stream(stream)))

    def read_line(self, channel, offset=0, count=None, stream=None):
        n = self.capacity - offset if count is None else count
        a = np.empty(n, np.float32)
        check(lib.mi_dyndelay_bank_read_line(self.handle, channel, a.ctypes.data_as(c_void_p), offset, n, _stream(stream)))
        return a

    def write_line(self, channel, values, offset=0, stream=None):
        a = np.ascontiguousarray(values, dtype=np.float32)
        check(lib.mi_dyndelay_bank_write_line(self.handle, channel, a.ctypes.data_as(c_void_p), offset, a.size, _stream(stream)))

    def count_steps(self, on=True, stream=None):
        """Debug counters of the kernel: switched on (and zeroed) or off."""
        check(lib.mi_dyndelay_bank_count_steps(self.handle, 1 if on else 0, _stream(stream)))

    def steps(self, stream=None):
        """(steps that ran one per lane, steps in all) since count_steps()."""
        p, t = ctypes.c_uint64(), ctypes.c_uint64()
        check(lib.mi_dyndelay_bank_steps(self.handle, byref(p), byref(t), _stream(stream)))
        return p.value, t.value

    def close(self):
        if self.handle:
            lib.mi_dyndelay_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class OscillatorBank:
    """`channels` x lsp::dspu::Oscillator (mi_oscillator_bank_*): phase-accumulator waveforms; nPhaseAcc on the device."""
    OVERWRITE, ADD, MUL = 0, 1, 2
    SETTERS = ("function", "frequency", "sample_rate", "phase", "phase_accumulator_bits", "dc_offset", "dc_reference", "amplitude",
               "duty_ratio", "width", "trapezoid_ratios", "pulsetrain_ratios", "parabolic_width", "squared_sinusoid_inversion",
               "parabolic_inversion", "oversampler_mode")

    def __init__(self, channels):
        h = c_void_p()
        check(lib.mi_oscillator_bank_create(byref(h), channels))
        self.handle, self.channels = h, channels

    def set(self, channel, setter, a=0.0, b=0.0):
        """One setter by its MI_OSC_SET_* number."""
        check(lib.mi_oscillator_bank_set(self.handle, channel, setter, float(a), float(b)))

    def __getattr__(self, name):
        # set_<name>(channel, value[, second]): the reference's setters, each one its own C entry
        if name.startswith("set_") and name[4:] in self.SETTERS:
            fn = getattr(lib, "mi_oscillator_bank_" + name)
            return lambda channel, *values: check(fn(self.handle, channel, *values))
        raise AttributeError(name)

    def reset_phase_accumulator(self, channel):
        check(lib.mi_oscillator_bank_reset_phase_accumulator(self.handle, channel))

    def needs_update(self, channel):
        v = c_int()
        check(lib.mi_oscillator_bank_needs_update(self.handle, channel, byref(v)))
        return bool(v.value)

    def update_settings(self, stream=None):
        check(lib.mi_oscillator_bank_update_settings(self.handle, _stream(stream)))

    def get_settings(self, channel):
        from .capi import OscillatorSettings
        s = OscillatorSettings()
        check(lib.mi_oscillator_bank_get_settings(self.handle, channel, byref(s)))
        return s

    def set_settings(self, channel, settings):
        check(lib.mi_oscillator_bank_set_settings(self.handle, channel, byref(settings)))

    def get_exact_frequency(self, channel):
        v = c_float()
        check(lib.mi_oscillator_bank_get_exact_frequency(self.handle, channel, byref(v)))
        return v.value

    def get_exact_phase(self, channel):
        v = c_float()
        check(lib.mi_oscillator_bank_get_exact_phase(self.handle, channel, byref(v)))
        return v.value

    def process(self, dst, count, src=None, op=0, dst_stride=None, src_stride=None, stream=None):
        """process_overwrite / process_add / process_mul by `op`; dst may be src (same stride); src may be None."""
        check(lib.mi_oscillator_bank_process(self.handle, _opt(dst), _opt(src), count, count if dst_stride is None else dst_stride,
                                             count if src_stride is None else src_stride, op, _stream(stream)))

    def reserve(self, count):
        check(lib.mi_oscillator_bank_reserve(self.handle, count))

    def set_exact(self, on=True):
        check(lib.mi_oscillator_bank_set_exact(self.handle, 1 if on else 0))

    def get_state(self, channel, stream=None):
        from .capi import OscillatorState
        s = OscillatorState()
        check(lib.mi_oscillator_bank_get_state(self.handle, channel, byref(s), _stream(stream)))
        return {"phase": s.phase}

    def set_state(self, channel, phase, stream=None):
        from .capi import OscillatorState
        s = OscillatorState(int(phase))
        check(lib.mi_oscillator_bank_set_state(self.handle, channel, byref(s), _stream(stream)))

    def get_periods(self, channel, dst, periods, skip, samples, stream=None):
        """get_periods(dst, periods, periodsSkip, samples) of one channel into a device row; synchronous."""
        check(lib.mi_oscillator_bank_get_periods(self.handle, channel, _opt(dst), periods, skip, samples, _stream(stream)))

    def synth_rows(self):
        """(device pointer, stride) of the oversampled rows of the last BL call."""
        p, n = c_void_p(), ctypes.c_size_t()
        check(lib.mi_oscillator_bank_synth_rows(self.handle, byref(p), byref(n)))
        return p.value or 0, n.value

    def close(self):
        if self.handle:
            lib.mi_oscillator_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ADSREnvelopeBank:
    """`channels` x lsp::dspu::ADSREnvelope (mi_adsr_bank_*): envelope curves over rows of time values, or generated from a start
    and a step per channel.  The unit has no state; every call can be captured (generate* replay the start and step of capture time)."""
    NONE, LINE, LINE2, CUBIC, QUADRO, EXP = range(6)
    SETTERS = ("attack_time", "hold_time", "decay_time", "slope_time", "release_time", "attack_curve", "decay_curve", "slope_curve",
               "release_curve", "attack_function", "decay_function", "slope_function", "release_function", "break_level",
               "sustain_level", "hold_enabled", "break_enabled", "attack", "hold", "decay", "break", "slope", "release")

    def __init__(self, channels):
        h = c_void_p()
        check(lib.mi_adsr_bank_create(byref(h), channels))
        self.handle, self.channels = h, channels

    def set(self, channel, setter, a=0.0, b=0.0, c=0.0):
        """One setter by its MI_ADSR_SET_* number."""
        check(lib.mi_adsr_bank_set(self.handle, channel, setter, float(a), float(b), float(c)))

    def __getattr__(self, name):
        # set_<name>(channel, value...): the reference's setters, each one its own C entry
        if name.startswith("set_") and name[4:] in self.SETTERS:
            fn = getattr(lib, "mi_adsr_bank_" + name)
            return lambda channel, *values: check(fn(self.handle, channel, *values))
        raise AttributeError(name)

    def needs_update(self, channel):
        v = c_int()
        check(lib.mi_adsr_bank_needs_update(self.handle, channel, byref(v)))
        return bool(v.value)

    def update_settings(self, stream=None):
        check(lib.mi_adsr_bank_update_settings(self.handle, _stream(stream)))

    def get_settings(self, channel):
        from .capi import AdsrSettings
        s = AdsrSettings()
        check(lib.mi_adsr_bank_get_settings(self.handle, channel, byref(s)))
        return s

    def set_settings(self, channel, settings):
        check(lib.mi_adsr_bank_set_settings(self.handle, channel, byref(settings)))

    def set_row_enabled(self, channel, enabled=True):
        check(lib.mi_adsr_bank_set_row_enabled(self.handle, channel, 1 if enabled else 0))

    def _pairs(self, start, step):
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(start, np.float32), (self.channels,)))
        b = np.ascontiguousarray(np.broadcast_to(np.asarray(step, np.float32), (self.channels,)))
        return a, b

    def process(self, dst, src, count, dst_stride=None, src_stride=None, stream=None):
        """dst[i] = do_process(src[i]); dst may be src (same stride)."""
        check(lib.mi_adsr_bank_process(self.handle, _opt(dst), _opt(src), count, count if dst_stride is None else dst_stride,
                                       count if src_stride is None else src_stride, _stream(stream)))

    def process_mul(self, dst, src, count, dst_stride=None, src_stride=None, stream=None):
        """dst[i] *= do_process(src[i])."""
        check(lib.mi_adsr_bank_process_mul(self.handle, _opt(dst), _opt(src), count, count if dst_stride is None else dst_stride,
                                           count if src_stride is None else src_stride, _stream(stream)))

    def generate(self, dst, start, step, count, dst_stride=None, stream=None):
        """The curve at t_i = start + i * step, one start and step per channel (a scalar serves all)."""
        a, b = self._pairs(start, step)
        check(lib.mi_adsr_bank_generate(self.handle, _opt(dst), a.ctypes.data_as(c_void_p), b.ctypes.data_as(c_void_p), count,
                                        count if dst_stride is None else dst_stride, _stream(stream)))

    def generate_mul(self, dst, start, step, count, src=None, dst_stride=None, src_stride=None, stream=None):
        """dst[i] *= the curve (src None) or dst[i] = src[i] * the curve; hold leaves or copies the sample, outside [0, 1] stores 0."""
        a, b = self._pairs(start, step)
        check(lib.mi_adsr_bank_generate_mul(self.handle, _opt(dst), _opt(src), a.ctypes.data_as(c_void_p), b.ctypes.data_as(c_void_p), count,
                                            count if dst_stride is None else dst_stride, count if src_stride is None else src_stride,
                                            _stream(stream)))

    def close(self):
        if self.handle:
            lib.mi_adsr_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LCGBank:
    """`channels` x lsp::dspu::LCG (mi_lcg_bank_*): white noise of four distributions; the Randomizers live on the device."""
    OVERWRITE, ADD, MUL = 0, 1, 2
    UNIFORM, EXPONENTIAL, TRIANGULAR, GAUSSIAN = 0, 1, 2, 3
    UNSET = 0xFFFFFFFF

    def __init__(self, channels):
        h = c_void_p()
        check(lib.mi_lcg_bank_create(byref(h), channels))
        self.handle, self.channels = h, channels

    def init(self, channel, seed=None):
        """init(seed); without a seed the argument-less init(): the host clock."""
        if seed is None:
            check(lib.mi_lcg_bank_init_time(self.handle, channel))
        else:
            check(lib.mi_lcg_bank_init(self.handle, channel, int(seed) & 0xFFFFFFFF))

    def set_distribution(self, channel, distribution):
        check(lib.mi_lcg_bank_set_distribution(self.handle, channel, distribution))

    def set_amplitude(self, channel, amplitude):
        check(lib.mi_lcg_bank_set_amplitude(self.handle, channel, amplitude))

    def set_offset(self, channel, offset):
        check(lib.mi_lcg_bank_set_offset(self.handle, channel, offset))

    def process(self, dst, count, src=None, op=0, dst_stride=None, src_stride=None, stream=None):
        """process_overwrite / process_add / process_mul by `op`; dst may be src (same stride)."""
        check(lib.mi_lcg_bank_process(self.handle, _opt(dst), _opt(src), count, count if dst_stride is None else dst_stride,
                                      count if src_stride is None else src_stride, op, _stream(stream)))

    def set_row_enabled(self, channel, enabled=True):
        """A channel that is switched off is skipped by process(): row not written, state and pending state kept."""
        check(lib.mi_lcg_bank_set_row_enabled(self.handle, channel, 1 if enabled else 0))

    def get_state(self, channel, stream=None):
        from .capi import LcgState
        s = LcgState()
        check(lib.mi_lcg_bank_get_state(self.handle, channel, byref(s), _stream(stream)))
        return {"last": list(s.last), "mul1": list(s.mul1), "mul2": list(s.mul2), "add": list(s.add), "buf_id": s.buf_id}

    def set_state(self, channel, last, mul1, mul2, add, buf_id, stream=None):
        from .capi import LcgState
        s = LcgState()
        for k in range(4):
            s.last[k], s.mul1[k], s.mul2[k], s.add[k] = int(last[k]), int(mul1[k]), int(mul2[k]), int(add[k])
        s.buf_id = int(buf_id) & 0xFFFFFFFF
        check(lib.mi_lcg_bank_set_state(self.handle, channel, byref(s), _stream(stream)))

    def close(self):
        if self.handle:
            lib.mi_lcg_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VelvetBank:
    """`channels` x lsp::dspu::Velvet (mi_velvet_bank_*): sparse-impulse noise; Randomizer and MLS of a channel live on the device."""
    OVERWRITE, ADD, MUL = 0, 1, 2
    CORE_MLS, CORE_LCG = 0, 1
    OVN, OVNA, ARN, TRN = 0, 1, 2, 3
    UNSET = 0xFFFFFFFF
    MAX_COUNT = 1 << 24

    def __init__(self, channels):
        h = c_void_p()
        check(lib.mi_velvet_bank_create(byref(h), channels))
        self.handle, self.channels = h, channels

    def init(self, channel, randseed=None, mls_n_bits=64, mls_seed=0):
        """init(randseed, mlsnbits, mlsseed); without a seed the argument-less init(): the host clock, and the MLS keeps what it has."""
        if randseed is None:
            check(lib.mi_velvet_bank_init_time(self.handle, channel))
        else:
            check(lib.mi_velvet_bank_init(self.handle, channel, int(randseed) & 0xFFFFFFFF, int(mls_n_bits) & 0xFF,
                                          int(mls_seed) & 0xFFFFFFFFFFFFFFFF))

    def set_core_type(self, channel, core):
        check(lib.mi_velvet_bank_set_core_type(self.handle, channel, core))

    def set_velvet_type(self, channel, type_):
        check(lib.mi_velvet_bank_set_velvet_type(self.handle, channel, type_))

    def set_velvet_window_width(self, channel, width):
        check(lib.mi_velvet_bank_set_velvet_window_width(self.handle, channel, width))

    def set_delta_value(self, channel, delta):
        check(lib.mi_velvet_bank_set_delta_value(self.handle, channel, delta))

    def set_crush_probability(self, channel, prob):
        check(lib.mi_velvet_bank_set_crush_probability(self.handle, channel, prob))

    def set_amplitude(self, channel, amplitude):
        check(lib.mi_velvet_bank_set_amplitude(self.handle, channel, amplitude))

    def set_offset(self, channel, offset):
        check(lib.mi_velvet_bank_set_offset(self.handle, channel, offset))

    def set_crush(self, channel, crush):
        check(lib.mi_velvet_bank_set_crush(self.handle, channel, int(bool(crush))))

    def process(self, dst, count, src=None, op=0, dst_stride=None, src_stride=None, stream=None):
        """process_overwrite / process_add / process_mul by `op`; src may be None with add (one segment) and mul (zero fill)."""
        check(lib.mi_velvet_bank_process(self.handle, _opt(dst), _opt(src), count, count if dst_stride is None else dst_stride,
                                         count if src_stride is None else src_stride, op, _stream(stream)))

    def process_segmented(self, dst, count, dst_stride=None, stream=None):
        """An overwrite in segments of 256 samples: a loop of process_overwrite(tmp, <= 256) in one launch."""
        check(lib.mi_velvet_bank_process_segmented(self.handle, _opt(dst), count, count if dst_stride is None else dst_stride, _stream(stream)))

    def set_row_enabled(self, channel, enabled=True):
        """A channel that is switched off is skipped by process(): row not written, state and pending state kept."""
        check(lib.mi_velvet_bank_set_row_enabled(self.handle, channel, 1 if enabled else 0))

    def reserve(self, count):
        check(lib.mi_velvet_bank_reserve(self.handle, count))

    def get_state(self, channel, stream=None):
        """The channel's VelvetState (capi): .rand as LcgState, .mls as MlsSettings."""
        from .capi import VelvetState
        s = VelvetState()
        check(lib.mi_velvet_bank_get_state(self.handle, channel, byref(s), _stream(stream)))
        return s

    def set_state(self, channel, state, stream=None):
        check(lib.mi_velvet_bank_set_state(self.handle, channel, byref(state), _stream(stream)))

    def close(self):
        if self.handle:
            lib.mi_velvet_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MLSBank:
    """`channels` x lsp::dspu::MLS (mi_mls_bank_*): maximum-length sequences of a register of 1 .. 64 bits; nState on the device."""
    OVERWRITE, ADD, MUL = 0, 1, 2

    def __init__(self, channels):
        h = c_void_p()
        check(lib.mi_mls_bank_create(byref(h), channels))
        self.handle, self.channels = h, channels

    def set_n_bits(self, channel, n_bits):
        check(lib.mi_mls_bank_set_n_bits(self.handle, channel, n_bits))

    def set_state(self, channel, state):
        check(lib.mi_mls_bank_set_state(self.handle, channel, int(state) & 0xFFFFFFFFFFFFFFFF))

    def set_amplitude(self, channel, amplitude):
        check(lib.mi_mls_bank_set_amplitude(self.handle, channel, amplitude))

    def set_offset(self, channel, offset):
        check(lib.mi_mls_bank_set_offset(self.handle, channel, offset))

    def needs_update(self, channel):
        v = c_int()
        check(lib.mi_mls_bank_needs_update(self.handle, channel, byref(v)))
        return bool(v.value)

    def update_settings(self, stream=None):
        check(lib.mi_mls_bank_update_settings(self.handle, _stream(stream)))

    def maximum_number_of_bits(self):
        v = ctypes.c_size_t()
        check(lib.mi_mls_bank_maximum_number_of_bits(self.handle, byref(v)))
        return v.value

    def get_period(self, channel):
        v = ctypes.c_uint64()
        check(lib.mi_mls_bank_get_period(self.handle, channel, byref(v)))
        return v.value

    def process(self, dst, count, src=None, op=0, dst_stride=None, src_stride=None, stream=None):
        """process_overwrite / process_add / process_mul by `op`; dst may be src (same stride)."""
        check(lib.mi_mls_bank_process(self.handle, _opt(dst), _opt(src), count, count if dst_stride is None else dst_stride,
                                      count if src_stride is None else src_stride, op, _stream(stream)))

    def set_row_enabled(self, channel, enabled=True):
        """A channel that is switched off is skipped by process(): row not written, nState and a pending update kept."""
        check(lib.mi_mls_bank_set_row_enabled(self.handle, channel, 1 if enabled else 0))

    def reserve(self, count):
        check(lib.mi_mls_bank_reserve(self.handle, count))

    def get_settings(self, channel):
        from .capi import MlsSettings
        s = MlsSettings()
        check(lib.mi_mls_bank_get_settings(self.handle, channel, byref(s)))
        return s

    def get_state(self, channel, stream=None):
        v = ctypes.c_uint64()
        check(lib.mi_mls_bank_get_state(self.handle, channel, byref(v), _stream(stream)))
        return v.value

    def close(self):
        if self.handle:
            lib.mi_mls_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _chart(call, f, packed):
    """freq_chart in either form on host arrays: complex64 [len(f)]."""
    f = np.ascontiguousarray(f, dtype=np.float32)
    if packed:
        c = np.empty(2 * f.size, np.float32)
        call(True, c.ctypes.data_as(c_void_p), None, f.ctypes.data_as(c_void_p), f.size)
        return c[0::2] + 1j * c[1::2]
    re, im = np.empty(f.size, np.float32), np.empty(f.size, np.float32)
    call(False, re.ctypes.data_as(c_void_p), im.ctypes.data_as(c_void_p), f.ctypes.data_as(c_void_p), f.size)
    return re + 1j * im


class SpectralTiltBank:
    """`channels` x lsp::dspu::SpectralTilt (mi_spectral_tilt_bank_*): a pole / zero cascade of up to 64 biquads that tilts the spectrum."""
    OVERWRITE, ADD, MUL = 0, 1, 2
    NEPER_PER_NEPER, DB_PER_OCTAVE, DB_PER_DECADE, UNIT_NONE = 0, 1, 2, 3
    NORM_AT_DC, NORM_AT_20_HZ, NORM_AT_1_KHZ, NORM_AT_20_KHZ, NORM_AT_NYQUIST, NORM_AUTO, NORM_NONE = range(7)
    MAX_SECTIONS = 64

    def __init__(self, channels):
        h = c_void_p()
        check(lib.mi_spectral_tilt_bank_create(byref(h), channels))
        self.handle, self.channels = h, channels

    def set_order(self, channel, order):
        check(lib.mi_spectral_tilt_bank_set_order(self.handle, channel, order))

    def set_slope(self, channel, slope, unit=0):
        check(lib.mi_spectral_tilt_bank_set_slope(self.handle, channel, slope, unit))

    def set_norm(self, channel, norm):
        check(lib.mi_spectral_tilt_bank_set_norm(self.handle, channel, norm))

    def set_lower_frequency(self, channel, lower):
        check(lib.mi_spectral_tilt_bank_set_lower_frequency(self.handle, channel, lower))

    def set_upper_frequency(self, channel, upper):
        check(lib.mi_spectral_tilt_bank_set_upper_frequency(self.handle, channel, upper))

    def set_frequency_range(self, channel, lower, upper):
        check(lib.mi_spectral_tilt_bank_set_frequency_range(self.handle, channel, lower, upper))

    def set_sample_rate(self, channel, sample_rate):
        check(lib.mi_spectral_tilt_bank_set_sample_rate(self.handle, channel, sample_rate))

    def set_row_enabled(self, channel, enabled=True):
        check(lib.mi_spectral_tilt_bank_set_row_enabled(self.handle, channel, 1 if enabled else 0))

    def set_exact(self, on=True):
        check(lib.mi_spectral_tilt_bank_set_exact(self.handle, 1 if on else 0))

    def update_settings(self, stream=None):
        check(lib.mi_spectral_tilt_bank_update_settings(self.handle, _stream(stream)))

    def commit(self, stream=None):
        check(lib.mi_spectral_tilt_bank_commit(self.handle, _stream(stream)))

    def reserve(self, count, stream=None):
        check(lib.mi_spectral_tilt_bank_reserve(self.handle, count, _stream(stream)))

    def process(self, dst, count, src=None, op=0, dst_stride=None, src_stride=None, stream=None):
        """process_overwrite / process_add / process_mul by `op`: dst = filter(src), dst += filter(src), dst *= filter(src)."""
        check(lib.mi_spectral_tilt_bank_process(self.handle, _opt(dst), _opt(src), count, count if dst_stride is None else dst_stride,
                                                count if src_stride is None else src_stride, op, _stream(stream)))

    def get_chains(self, channel):
        """(n, 5) float32 {b0, b1, b2, a1, a2}: the sections as the channel's last update_settings() left them."""
        arr, n = (BiquadX1 * self.MAX_SECTIONS)(), c_uint32()
        check(lib.mi_spectral_tilt_bank_get_chains(self.handle, channel, arr, byref(n)))
        return np.frombuffer(arr, np.float32).reshape(self.MAX_SECTIONS, 8)[:n.value, :5].copy()

    def get_settings(self, channel):
        from .capi import SpectralTiltSettings
        s = SpectralTiltSettings()
        check(lib.mi_spectral_tilt_bank_get_settings(self.handle, channel, byref(s)))
        return s

    def freq_chart(self, channel, f, packed=False):
        def call(p, a, b, fp, n):
            if p:
                check(lib.mi_spectral_tilt_bank_freq_chart_packed(self.handle, channel, a, fp, n))
            else:
                check(lib.mi_spectral_tilt_bank_freq_chart(self.handle, channel, a, b, fp, n))
        return _chart(call, f, packed)

    def reset(self, channel=None, stream=None):
        check(lib.mi_spectral_tilt_bank_reset(self.handle, 0xFFFFFFFF if channel is None else channel, _stream(stream)))

    def get_state(self, channel, stream=None):
        st = np.empty((self.MAX_SECTIONS, 2), np.float32)
        check(lib.mi_spectral_tilt_bank_get_state(self.handle, channel, st.ctypes.data_as(c_void_p), _stream(stream)))
        return st

    def set_state(self, channel, state, stream=None):
        st = np.ascontiguousarray(state, dtype=np.float32)
        assert st.shape == (self.MAX_SECTIONS, 2)
        check(lib.mi_spectral_tilt_bank_set_state(self.handle, channel, st.ctypes.data_as(c_void_p), _stream(stream)))

    def close(self):
        if self.handle:
            lib.mi_spectral_tilt_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NoiseGeneratorBank:
    """`channels` x lsp::dspu::NoiseGenerator (mi_noise_generator_bank_*): MLS, LCG and Velvet noise behind one interface, coloured
    by a SpectralTilt."""
    OVERWRITE, ADD, MUL = 0, 1, 2
    GEN_MLS, GEN_LCG, GEN_VELVET = 0, 1, 2
    WHITE, PINK, RED, BLUE, VIOLET, ARBITRARY = range(6)

    def __init__(self, channels):
        h = c_void_p()
        check(lib.mi_noise_generator_bank_create(byref(h), channels))
        self.handle, self.channels = h, channels

    def init(self, channel, mls_n_bits=None, mls_seed=0, lcg_seed=0, velvet_rand_seed=0, velvet_mls_n_bits=0, velvet_mls_seed=0):
        """init(...) with its six arguments; without any the argument-less init(): time seeds, an MLS of 64 bits."""
        if mls_n_bits is None:
            check(lib.mi_noise_generator_bank_init_auto(self.handle, channel))
        else:
            check(lib.mi_noise_generator_bank_init(self.handle, channel, int(mls_n_bits) & 0xFF, int(mls_seed) & 0xFFFFFFFFFFFFFFFF,
                                                   int(lcg_seed) & 0xFFFFFFFF, int(velvet_rand_seed) & 0xFFFFFFFF,
                                                   int(velvet_mls_n_bits) & 0xFF, int(velvet_mls_seed) & 0xFFFFFFFFFFFFFFFF))

    def _set(self, name, channel, *args):
        check(getattr(lib, "mi_noise_generator_bank_set_" + name)(self.handle, channel, *args))

    def set_sample_rate(self, channel, sr): self._set("sample_rate", channel, sr)
    def set_mls_n_bits(self, channel, n): self._set("mls_n_bits", channel, int(n) & 0xFF)
    def set_mls_seed(self, channel, seed): self._set("mls_seed", channel, int(seed) & 0xFFFFFFFFFFFFFFFF)
    def set_lcg_distribution(self, channel, dist): self._set("lcg_distribution", channel, dist)
    def set_velvet_type(self, channel, type_): self._set("velvet_type", channel, type_)
    def set_velvet_window_width(self, channel, seconds): self._set("velvet_window_width", channel, seconds)
    def set_velvet_arn_delta(self, channel, delta): self._set("velvet_arn_delta", channel, delta)
    def set_velvet_crush(self, channel, crush): self._set("velvet_crush", channel, int(bool(crush)))
    def set_velvet_crushing_probability(self, channel, prob): self._set("velvet_crushing_probability", channel, prob)
    def set_generator(self, channel, generator): self._set("generator", channel, generator)
    def set_noise_color(self, channel, color): self._set("noise_color", channel, color)
    def set_coloring_order(self, channel, order): self._set("coloring_order", channel, order)
    def set_color_slope(self, channel, slope, unit=0): self._set("color_slope", channel, slope, unit)
    def set_amplitude(self, channel, amplitude): self._set("amplitude", channel, amplitude)
    def set_offset(self, channel, offset): self._set("offset", channel, offset)

    def set_exact(self, on=True):
        check(lib.mi_noise_generator_bank_set_exact(self.handle, 1 if on else 0))

    def update_settings(self, stream=None):
        check(lib.mi_noise_generator_bank_update_settings(self.handle, _stream(stream)))

    def reserve(self, count, stream=None):
        check(lib.mi_noise_generator_bank_reserve(self.handle, count, _stream(stream)))

    def process(self, dst, count, src=None, op=0, dst_stride=None, src_stride=None, stream=None):
        """process_overwrite / process_add / process_mul by `op`; src may be None with add (as overwrite) and mul (zero fill)."""
        check(lib.mi_noise_generator_bank_process(self.handle, _opt(dst), _opt(src), count, count if dst_stride is None else dst_stride,
                                                  count if src_stride is None else src_stride, op, _stream(stream)))

    def freq_chart(self, channel, f, packed=False):
        def call(p, a, b, fp, n):
            if p:
                check(lib.mi_noise_generator_bank_freq_chart_packed(self.handle, channel, a, fp, n))
            else:
                check(lib.mi_noise_generator_bank_freq_chart(self.handle, channel, a, b, fp, n))
        return _chart(call, f, packed)

    def get_settings(self, channel):
        from .capi import NoiseGeneratorSettings
        s = NoiseGeneratorSettings()
        check(lib.mi_noise_generator_bank_get_settings(self.handle, channel, byref(s)))
        return s

    def get_tilt_settings(self, channel):
        from .capi import SpectralTiltSettings
        s = SpectralTiltSettings()
        check(lib.mi_noise_generator_bank_get_tilt_settings(self.handle, channel, byref(s)))
        return s

    def get_state(self, channel, stream=None):
        from .capi import NoiseGeneratorState
        s = NoiseGeneratorState()
        check(lib.mi_noise_generator_bank_get_state(self.handle, channel, byref(s), _stream(stream)))
        return s

    def set_state(self, channel, state, stream=None):
        check(lib.mi_noise_generator_bank_set_state(self.handle, channel, byref(state), _stream(stream)))

    def close(self):
        if self.handle:
            lib.mi_noise_generator_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RingBank:
    """`channels` x lsp::dspu::RingBuffer on the device."""

    def __init__(self, channels, size, fill=0.0):
        h = c_void_p()
        check(lib.mi_ring_bank_create(byref(h), channels, size, fill))
        self.handle, self.channels = h, channels

    def fill(self, value=0.0, stream=None):
        check(lib.mi_ring_bank_fill(self.handle, value, _stream(stream)))

    def append(self, inp, count, in_stride=None, stream=None):
        n = ctypes.c_size_t()
        check(lib.mi_ring_bank_append(self.handle, _ptr(inp), count, count if in_stride is None else in_stride,
                                      byref(n), _stream(stream)))
        return n.value

    def get(self, out, offset, count, out_stride=None, stream=None):
        n = ctypes.c_size_t()
        check(lib.mi_ring_bank_get(self.handle, _ptr(out), offset, count, count if out_stride is None else out_stride,
                                   byref(n), _stream(stream)))
        return n.value

    def info(self, offset=0):
        v = [c_uint32() for _ in range(3)]
        check(lib.mi_ring_bank_info(self.handle, offset, *[byref(x) for x in v]))
        return dict(zip(("capacity", "head", "tail_position"), [x.value for x in v]))

    def close(self):
        if self.handle:
            lib.mi_ring_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TruePeakBank:
    """`channels` x lsp::dspu::TruePeakMeter (mi_truepeak_bank_*): BS.1770-4 true peak per sample, or its maximum per call."""

    def __init__(self, channels):
        h = c_void_p()
        check(lib.mi_truepeak_bank_create(byref(h), channels))
        self.handle, self.channels = h, channels

    @staticmethod
    def coefficients(times):
        """The kernels' table for `times` (mi_truepeak_coefficients): float32 [times][20], row k the phase k / times."""
        n = ctypes.c_size_t()
        check(lib.mi_truepeak_coefficients(times, None, byref(n)))
        h = np.zeros(n.value, np.float32)
        check(lib.mi_truepeak_coefficients(times, h.ctypes.data_as(ctypes.POINTER(c_float)), byref(n)))
        return h.reshape(times, 20) if times else h.reshape(0, 20)

    def set_sample_rate(self, sr):
        check(lib.mi_truepeak_bank_set_sample_rate(self.handle, sr))

    def update_settings(self, stream=None):
        check(lib.mi_truepeak_bank_update_settings(self.handle, _stream(stream)))

    def clear(self, stream=None):
        check(lib.mi_truepeak_bank_clear(self.handle, _stream(stream)))

    def latency(self):
        v = c_uint32()
        check(lib.mi_truepeak_bank_latency(self.handle, byref(v)))
        return v.value

    def oversampling(self):
        v = c_uint32()
        check(lib.mi_truepeak_bank_oversampling(self.handle, byref(v)))
        return v.value

    def process(self, out, inp, count, out_stride=None, in_stride=None, stream=None):
        """process(dst, src, count); out may be inp (in place)."""
        check(lib.mi_truepeak_bank_process(self.handle, _ptr(out), _ptr(inp), count, count if out_stride is None else out_stride,
                                           count if in_stride is None else in_stride, _stream(stream)))

    def process_max(self, peaks, inp, count, in_stride=None, stream=None):
        """process_max(src, count) of every channel into the device array `peaks` [channels]."""
        check(lib.mi_truepeak_bank_process_max(self.handle, _ptr(peaks), _ptr(inp), count, count if in_stride is None else in_stride,
                                               _stream(stream)))

    def close(self):
        if self.handle:
            lib.mi_truepeak_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class OversamplerBank:
    """`channels` x lsp::dspu::Oversampler (mi_oversampler_bank_*): Lanczos upsampling, the caller's work on the oversampled
    rows, the anti-alias filter and the decimation."""
    # over_mode_t (util/Oversampler.h:62-100): OM_NONE, then LANCZOS_<N>X<K> for N in 2, 3, 4, 6, 8 and K as below
    OM_NONE = 0
    MODES = {"%dX%s" % (n, k): 1 + 6 * g + j for g, n in enumerate((2, 3, 4, 6, 8))
             for j, k in enumerate(("2", "3", "4", "12BIT", "16BIT", "24BIT"))}

    def __init__(self, channels):
        h = c_void_p()
        check(lib.mi_oversampler_bank_create(byref(h), channels))
        self.handle, self.channels = h, channels
        self._cb = None

    @staticmethod
    def coefficients(mode):
        """The kernels' table of `mode` (mi_oversampler_coefficients): float32 [N][2a], row k the phase k / N."""
        n = ctypes.c_size_t()
        check(lib.mi_oversampler_coefficients(mode, None, byref(n)))
        h = np.zeros(n.value, np.float32)
        if n.value:
            check(lib.mi_oversampler_coefficients(mode, h.ctypes.data_as(ctypes.POINTER(c_float)), byref(n)))
        times = 1 if mode == 0 else (2, 3, 4, 6, 8)[(mode - 1) // 6]
        return h.reshape(times, -1) if n.value else h.reshape(0, 0)

    def set_sample_rate(self, sr):
        check(lib.mi_oversampler_bank_set_sample_rate(self.handle, sr))

    def set_mode(self, mode):
        check(lib.mi_oversampler_bank_set_mode(self.handle, mode))

    def mode(self):
        v = c_uint32()
        check(lib.mi_oversampler_bank_mode(self.handle, byref(v)))
        return v.value

    def set_filtering(self, on=True):
        check(lib.mi_oversampler_bank_set_filtering(self.handle, 1 if on else 0))

    def filtering(self):
        v = c_int()
        check(lib.mi_oversampler_bank_filtering(self.handle, byref(v)))
        return bool(v.value)

    def modified(self):
        v = c_int()
        check(lib.mi_oversampler_bank_modified(self.handle, byref(v)))
        return bool(v.value)

    def update_settings(self, stream=None):
        check(lib.mi_oversampler_bank_update_settings(self.handle, _stream(stream)))

    def _u32(self, fn):
        v = c_uint32()
        check(fn(self.handle, byref(v)))
        return v.value

    def oversampling(self):
        return self._u32(lib.mi_oversampler_bank_oversampling)

    def latency(self):
        return self._u32(lib.mi_oversampler_bank_latency)

    def max_latency(self):
        return self._u32(lib.mi_oversampler_bank_max_latency)

    def reserve(self, count):
        check(lib.mi_oversampler_bank_reserve(self.handle, count))

    def set_exact(self, on=True):
        check(lib.mi_oversampler_bank_set_exact(self.handle, 1 if on else 0))

    def get_filter(self):
        """(filter parameters as a dict, the rate they are designed at)."""
        fp, sr = FilterParams(), c_uint32()
        check(lib.mi_oversampler_bank_get_filter(self.handle, byref(fp), byref(sr)))
        return {n: getattr(fp, n) for n, _ in FilterParams._fields_}, sr.value

    def upsample(self, out, inp, count, out_stride=None, in_stride=None, stream=None):
        """upsample(dst, src, count): out rows of N * count samples."""
        n = self.oversampling()
        check(lib.mi_oversampler_bank_upsample(self.handle, _ptr(out), _ptr(inp), count, n * count if out_stride is None else out_stride,
                                               count if in_stride is None else in_stride, _stream(stream)))

    def downsample(self, out, inp, count, out_stride=None, in_stride=None, stream=None):
        """downsample(dst, src, count): inp rows of N * count samples."""
        n = self.oversampling()
        check(lib.mi_oversampler_bank_downsample(self.handle, _ptr(out), _ptr(inp), count, count if out_stride is None else out_stride,
                                                 n * count if in_stride is None else in_stride, _stream(stream)))

    def process(self, out, inp, count, callback=None, out_stride=None, in_stride=None, stream=None):
        """process(dst, src, count, callback); out may be inp.  callback(buf_ptr, samples, stride, channels, stream) runs on
        the host once per call and enqueues its work on `stream` over the oversampled device rows, in place."""
        from .capi import OVERSAMPLER_FUNC
        cb = None
        if callback is not None:
            def _call(buf, samples, stride, channels, st, arg):
                r = callback(buf, samples, stride, channels, st)
                return 0 if r is None else int(r)
            cb = self._cb = OVERSAMPLER_FUNC(_call)
        check(lib.mi_oversampler_bank_process(self.handle, _ptr(out), _ptr(inp), count, count if out_stride is None else out_stride,
                                              count if in_stride is None else in_stride,
                                              ctypes.cast(cb, c_void_p) if cb is not None else None, None, _stream(stream)))

    def close(self):
        if self.handle:
            lib.mi_oversampler_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _DynamicsBank:
    """What the four envelope dynamics banks share: the calls of mi_<unit>_bank_* that have one signature."""
    UNIT = None

    def __init__(self, channels):
        h = c_void_p()
        check(self._fn("create")(byref(h), channels))
        self.handle, self.channels = h, channels

    @classmethod
    def _fn(cls, name):
        return getattr(lib, "mi_%s_bank_%s" % (cls.UNIT, name))

    def set_sample_rate(self, channel, sr):
        check(self._fn("set_sample_rate")(self.handle, channel, sr))

    def set_timings(self, channel, attack, release):
        check(self._fn("set_timings")(self.handle, channel, attack, release))

    def set_hold(self, channel, hold):
        check(self._fn("set_hold")(self.handle, channel, hold))

    def update_settings(self, stream=None):
        check(self._fn("update_settings")(self.handle, _stream(stream)))

    def clear(self, stream=None):
        check(self._fn("clear")(self.handle, _stream(stream)))

    def process(self, gain, env, inp, count, gain_stride=None, env_stride=None, in_stride=None, stream=None):
        """process(out, env, in, samples); env may be None, gain or env may be inp (in place)."""
        check(self._fn("process")(self.handle, _ptr(gain), None if env is None else _ptr(env), _ptr(inp), count,
                                  count if gain_stride is None else gain_stride, count if env_stride is None else env_stride,
                                  count if in_stride is None else in_stride, _stream(stream)))

    def process_apply(self, out, audio, sc, count, out_stride=None, audio_stride=None, sc_stride=None, stream=None):
        """out = audio * gain(sc) in one launch; out may be audio or sc."""
        check(self._fn("process_apply")(self.handle, _ptr(out), _ptr(audio), _ptr(sc), count,
                                        count if out_stride is None else out_stride,
                                        count if audio_stride is None else audio_stride,
                                        count if sc_stride is None else sc_stride, _stream(stream)))

    def close(self):
        if self.handle:
            self._fn("destroy")(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _params_dict(p):
    return {"tau_attack": p.tau_attack, "tau_release": p.tau_release, "release_threshold": p.release_threshold, "hold": p.hold,
            "k": [{"start": k.start, "end": k.end, "gain": k.gain, "herm": np.array(k.herm[:], np.float32),
                   "tilt": np.array(k.tilt[:], np.float32)} for k in p.k]}


class CompressorBank(_DynamicsBank):
    """`channels` x lsp::dspu::Compressor (mi_compressor_bank_*): envelope follower and two-knee gain curve, every channel
    with settings of its own."""
    UNIT = "compressor"
    CM_DOWNWARD, CM_UPWARD, CM_BOOSTING = range(3)

    @staticmethod
    def compute_params(sample_rate=0, mode=0, attack_threshold=0.0, release_threshold=0.0, boost_threshold=2.5119e-4, attack=0.0,
                       release=0.0, hold=0.0, knee=0.0, ratio=1.0):
        """update_settings() of one compressor on the host (mi_compressor_compute_params): no device needed."""
        from .capi import CompressorParams, CompressorSettings
        s = CompressorSettings(sample_rate, mode, attack_threshold, release_threshold, boost_threshold, attack, release, hold, knee, ratio)
        p = CompressorParams()
        check(lib.mi_compressor_compute_params(byref(s), byref(p)))
        return _params_dict(p)

    def set_mode(self, channel, mode):
        check(lib.mi_compressor_bank_set_mode(self.handle, channel, mode))

    def set_threshold(self, channel, attack, release):
        check(lib.mi_compressor_bank_set_threshold(self.handle, channel, attack, release))

    def set_boost_threshold(self, channel, boost):
        check(lib.mi_compressor_bank_set_boost_threshold(self.handle, channel, boost))

    def set_knee(self, channel, knee):
        check(lib.mi_compressor_bank_set_knee(self.handle, channel, knee))

    def set_ratio(self, channel, ratio):
        check(lib.mi_compressor_bank_set_ratio(self.handle, channel, ratio))

    def configure(self, channel, sample_rate, mode, attack_threshold, release_threshold, boost_threshold, attack, release, hold,
                  knee, ratio):
        """Every setter of one channel."""
        self.set_sample_rate(channel, sample_rate)
        self.set_mode(channel, mode)
        self.set_threshold(channel, attack_threshold, release_threshold)
        self.set_boost_threshold(channel, boost_threshold)
        self.set_timings(channel, attack, release)
        self.set_hold(channel, hold)
        self.set_knee(channel, knee)
        self.set_ratio(channel, ratio)

    def get_params(self, channel):
        from .capi import CompressorParams
        p = CompressorParams()
        check(lib.mi_compressor_bank_get_params(self.handle, channel, byref(p)))
        return _params_dict(p)

    def get_state(self, channel, stream=None):
        """(fEnvelope, fPeak, nHoldCounter) of the channel; the envelope and the peak as numpy float32."""
        e, p, h = c_float(), c_float(), c_uint32()
        check(lib.mi_compressor_bank_get_state(self.handle, channel, byref(e), byref(p), byref(h), _stream(stream)))
        return np.float32(e.value), np.float32(p.value), h.value

    def curve(self, out, inp, dots, out_stride=None, in_stride=None, stream=None):
        """curve(out, in, dots) of every channel: out = gain(|in|) |in|."""
        check(lib.mi_compressor_bank_curve(self.handle, _ptr(out), _ptr(inp), dots, dots if out_stride is None else out_stride,
                                           dots if in_stride is None else in_stride, _stream(stream)))


def _expander_dict(p):
    return {"tau_attack": p.tau_attack, "tau_release": p.tau_release, "release_threshold": p.release_threshold, "hold": p.hold,
            "upward": p.upward,
            "k": {"start": p.k.start, "end": p.k.end, "threshold": p.k.threshold, "herm": np.array(p.k.herm[:], np.float32),
                  "tilt": np.array(p.k.tilt[:], np.float32)}}


class ExpanderBank(_DynamicsBank):
    """`channels` x lsp::dspu::Expander (mi_expander_bank_*): envelope follower and one-knee gain curve, upward or downward,
    every channel with settings of its own."""
    UNIT = "expander"
    EM_DOWNWARD, EM_UPWARD = range(2)

    @staticmethod
    def compute_params(sample_rate=0, mode=1, attack_threshold=0.0, release_threshold=0.0, attack=0.0, release=0.0, hold=0.0,
                       knee=0.0, ratio=1.0):
        """update_settings() of one expander on the host (mi_expander_compute_params): no device needed."""
        from .capi import ExpanderParams, ExpanderSettings
        s = ExpanderSettings(sample_rate, mode, attack_threshold, release_threshold, attack, release, hold, knee, ratio)
        p = ExpanderParams()
        check(lib.mi_expander_compute_params(byref(s), byref(p)))
        return _expander_dict(p)

    def set_mode(self, channel, mode):
        check(lib.mi_expander_bank_set_mode(self.handle, channel, mode))

    def set_threshold(self, channel, attack, release):
        check(lib.mi_expander_bank_set_threshold(self.handle, channel, attack, release))

    def set_knee(self, channel, knee):
        check(lib.mi_expander_bank_set_knee(self.handle, channel, knee))

    def set_ratio(self, channel, ratio):
        check(lib.mi_expander_bank_set_ratio(self.handle, channel, ratio))

    def configure(self, channel, sample_rate, mode, attack_threshold, release_threshold, attack, release, hold, knee, ratio):
        """Every setter of one channel."""
        self.set_sample_rate(channel, sample_rate)
        self.set_mode(channel, mode)
        self.set_threshold(channel, attack_threshold, release_threshold)
        self.set_timings(channel, attack, release)
        self.set_hold(channel, hold)
        self.set_knee(channel, knee)
        self.set_ratio(channel, ratio)

    def get_params(self, channel):
        from .capi import ExpanderParams
        p = ExpanderParams()
        check(lib.mi_expander_bank_get_params(self.handle, channel, byref(p)))
        return _expander_dict(p)

    def get_state(self, channel, stream=None):
        """(fEnvelope, fPeak, nHoldCounter) of the channel; the envelope and the peak as numpy float32."""
        e, p, h = c_float(), c_float(), c_uint32()
        check(lib.mi_expander_bank_get_state(self.handle, channel, byref(e), byref(p), byref(h), _stream(stream)))
        return np.float32(e.value), np.float32(p.value), h.value

    def curve(self, out, inp, dots, out_stride=None, in_stride=None, stream=None):
        """curve(out, in, dots) of every channel."""
        check(lib.mi_expander_bank_curve(self.handle, _ptr(out), _ptr(inp), dots, dots if out_stride is None else out_stride,
                                         dots if in_stride is None else in_stride, _stream(stream)))


def _gate_dict(p):
    return {"tau_attack": p.tau_attack, "tau_release": p.tau_release, "hold": p.hold,
            "k": [{"start": k.start, "end": k.end, "gain_start": k.gain_start, "gain_end": k.gain_end,
                   "herm": np.array(k.herm[:], np.float32)} for k in p.k]}


class GateBank(_DynamicsBank):
    """`channels` x lsp::dspu::Gate (mi_gate_bank_*): envelope follower, an open and a close curve and the hysteresis between
    them, every channel with settings of its own."""
    UNIT = "gate"

    @staticmethod
    def compute_params(sample_rate=0, open_threshold=0.0, close_threshold=0.0, open_zone=1.0, close_zone=1.0, reduction=0.0,
                       attack=0.0, release=0.0, hold=0.0):
        """update_settings() of one gate on the host (mi_gate_compute_params): no device needed."""
        from .capi import GateParams, GateSettings
        s = GateSettings(sample_rate, (c_float * 2)(open_threshold, close_threshold), (c_float * 2)(open_zone, close_zone),
                         reduction, attack, release, hold)
        p = GateParams()
        check(lib.mi_gate_compute_params(byref(s), byref(p)))
        return _gate_dict(p)

    def set_threshold(self, channel, open, close):
        check(lib.mi_gate_bank_set_threshold(self.handle, channel, open, close))

    def set_zone(self, channel, open, close):
        check(lib.mi_gate_bank_set_zone(self.handle, channel, open, close))

    def set_reduction(self, channel, reduction):
        check(lib.mi_gate_bank_set_reduction(self.handle, channel, reduction))

    def configure(self, channel, sample_rate, open_threshold, close_threshold, open_zone, close_zone, reduction, attack, release,
                  hold):
        """Every setter of one channel."""
        self.set_sample_rate(channel, sample_rate)
        self.set_threshold(channel, open_threshold, close_threshold)
        self.set_zone(channel, open_zone, close_zone)
        self.set_reduction(channel, reduction)
        self.set_timings(channel, attack, release)
        self.set_hold(channel, hold)

    def get_params(self, channel):
        from .capi import GateParams
        p = GateParams()
        check(lib.mi_gate_bank_get_params(self.handle, channel, byref(p)))
        return _gate_dict(p)

    def get_state(self, channel, stream=None):
        """(fEnvelope, fPeak, nHoldCounter, nCurve) of the channel; the envelope and the peak as numpy float32."""
        e, p, h, c = c_float(), c_float(), c_uint32(), c_uint32()
        check(lib.mi_gate_bank_get_state(self.handle, channel, byref(e), byref(p), byref(h), byref(c), _stream(stream)))
        return np.float32(e.value), np.float32(p.value), h.value, c.value

    def curve(self, out, inp, dots, hyst=False, out_stride=None, in_stride=None, stream=None):
        """curve(out, in, dots, hyst) of every channel: the open curve, with hyst the close curve."""
        check(lib.mi_gate_bank_curve(self.handle, _ptr(out), _ptr(inp), dots, 1 if hyst else 0,
                                     dots if out_stride is None else out_stride, dots if in_stride is None else in_stride,
                                     _stream(stream)))


def _limiter_dict(p):
    d = dict((n, getattr(p, n)) for n in ("lookahead", "mode", "attack", "plane", "release", "middle"))
    d.update((n, np.float32(getattr(p, n))) for n in ("threshold", "ks", "ke", "gain", "tau_attack", "tau_release"))
    d.update((n, np.array(getattr(p, n)[:], np.float32)) for n in ("v_attack", "v_release", "hermite"))
    return d


def _limiter_params(d):
    from .capi import LimiterParams
    p = LimiterParams()
    for n in ("lookahead", "mode", "attack", "plane", "release", "middle", "threshold", "ks", "ke", "gain", "tau_attack", "tau_release"):
        setattr(p, n, d[n].item() if hasattr(d[n], "item") else d[n])
    for n in ("v_attack", "v_release", "hermite"):
        getattr(p, n)[:] = [float(v) for v in d[n]]
    return p


class LimiterBank:
    """`channels` x lsp::dspu::Limiter (mi_limiter_bank_*): look-ahead peak search and multiplicative gain patches, every
    channel with settings and mode of its own; the maximum sample rate and look-ahead (ms) are the bank's."""
    MODES = ("HERM_THIN", "HERM_WIDE", "HERM_TAIL", "HERM_DUCK", "EXP_THIN", "EXP_WIDE", "EXP_TAIL", "EXP_DUCK",
             "LINE_THIN", "LINE_WIDE", "LINE_TAIL", "LINE_DUCK")
    MAX_LOOKAHEAD = 4064
    SETTINGS = {"sample_rate": 0, "mode": 0, "threshold": 1.0, "lookahead": 0.0, "attack": 0.0, "release": 0.0, "knee": 0.50118,
                "alr_attack": 10.0, "alr_release": 50.0, "alr_knee": 0.56234}

    def __init__(self, channels, max_sample_rate, max_lookahead):
        h = c_void_p()
        check(lib.mi_limiter_bank_create(byref(h), channels, max_sample_rate, max_lookahead))
        self.handle, self.channels = h, channels

    @classmethod
    def compute_params(cls, **settings):
        """update_settings() of one limiter on the host (mi_limiter_compute_params): no device needed.  Keywords as SETTINGS
        (construct()'s values where not given); alr_knee is the stored value."""
        from .capi import LimiterParams, LimiterSettings
        v = dict(cls.SETTINGS, **settings)
        s = LimiterSettings(*[v[n] for n, _ in LimiterSettings._fields_])
        p = LimiterParams()
        check(lib.mi_limiter_compute_params(byref(s), byref(p)))
        return _limiter_dict(p)

    @staticmethod
    def compute_patch(params):
        """The patch of compute_params()'s result as a table of params["release"] float32 (mi_limiter_compute_patch)."""
        out = np.zeros(max(params["release"], 0), np.float32)
        check(lib.mi_limiter_compute_patch(byref(_limiter_params(params)), out.ctypes.data_as(c_void_p), out.size))
        return out

    def set_sample_rate(self, channel, sr):
        check(lib.mi_limiter_bank_set_sample_rate(self.handle, channel, sr))

    def set_mode(self, channel, mode):
        check(lib.mi_limiter_bank_set_mode(self.handle, channel, mode))

    def set_threshold(self, channel, threshold, immediate=False):
        check(lib.mi_limiter_bank_set_threshold(self.handle, channel, threshold, 1 if immediate else 0))

    def set_attack(self, channel, attack):
        check(lib.mi_limiter_bank_set_attack(self.handle, channel, attack))

    def set_release(self, channel, release):
        check(lib.mi_limiter_bank_set_release(self.handle, channel, release))

    def set_lookahead(self, channel, lookahead):
        check(lib.mi_limiter_bank_set_lookahead(self.handle, channel, lookahead))

    def set_knee(self, channel, knee):
        check(lib.mi_limiter_bank_set_knee(self.handle, channel, knee))

    def set_alr(self, channel, enable):
        check(lib.mi_limiter_bank_set_alr(self.handle, channel, 1 if enable else 0))

    def set_alr_attack(self, channel, attack):
        check(lib.mi_limiter_bank_set_alr_attack(self.handle, channel, attack))

    def set_alr_release(self, channel, release):
        check(lib.mi_limiter_bank_set_alr_release(self.handle, channel, release))

    def set_alr_knee(self, channel, knee):
        check(lib.mi_limiter_bank_set_alr_knee(self.handle, channel, knee))

    def configure(self, channel, sample_rate, mode, threshold, lookahead, attack, release, knee=None, alr=None, alr_attack=None,
                  alr_release=None, alr_knee=None, immediate=True):
        """The setters of one channel; what is None keeps its value."""
        self.set_sample_rate(channel, sample_rate)
        self.set_mode(channel, mode)
        self.set_threshold(channel, threshold, immediate)
        self.set_lookahead(channel, lookahead)
        self.set_attack(channel, attack)
        self.set_release(channel, release)
        for value, setter in ((knee, self.set_knee), (alr_attack, self.set_alr_attack), (alr_release, self.set_alr_release),
                              (alr_knee, self.set_alr_knee), (alr, self.set_alr)):
            if value is not None:
                setter(channel, value)

    def update_settings(self, stream=None):
        check(lib.mi_limiter_bank_update_settings(self.handle, _stream(stream)))

    def clear(self, stream=None):
        check(lib.mi_limiter_bank_clear(self.handle, _stream(stream)))

    def get_params(self, channel):
        from .capi import LimiterParams
        p = LimiterParams()
        check(lib.mi_limiter_bank_get_params(self.handle, channel, byref(p)))
        return _limiter_dict(p)

    def get_patch(self, channel, stream=None):
        """The channel's shape table as the device has it, float32."""
        out = np.zeros(3 * self.MAX_LOOKAHEAD + 17, np.float32)
        n = c_uint32()
        check(lib.mi_limiter_bank_get_patch(self.handle, channel, out.ctypes.data_as(c_void_p), out.size, byref(n), _stream(stream)))
        return out[:n.value].copy()

    def get_latency(self, channel):
        n = c_uint32()
        check(lib.mi_limiter_bank_get_latency(self.handle, channel, byref(n)))
        return n.value

    def get_state(self, channel, stream=None):
        """(nHead, sALR.fEnvelope as numpy float32, patches and chunks of the last call, the sticky overrun flag)."""
        h, e, p, c, o = c_uint32(), c_float(), c_uint32(), c_uint32(), c_uint32()
        check(lib.mi_limiter_bank_get_state(self.handle, channel, byref(h), byref(e), byref(p), byref(c), byref(o), _stream(stream)))
        return h.value, np.float32(e.value), p.value, c.value, o.value

    def process(self, gain, sc, count, gain_stride=None, sc_stride=None, stream=None):
        """process(gain, sc, samples); gain may be sc (in place)."""
        check(lib.mi_limiter_bank_process(self.handle, _ptr(gain), _ptr(sc), count, count if gain_stride is None else gain_stride,
                                          count if sc_stride is None else sc_stride, _stream(stream)))

    def process_apply(self, out, audio, sc, count, out_stride=None, audio_stride=None, sc_stride=None, stream=None):
        """out[i] = audio_stream[i - latency] * gain[i] in one launch; out may be audio or sc."""
        check(lib.mi_limiter_bank_process_apply(self.handle, _ptr(out), _ptr(audio), _ptr(sc), count,
                                                count if out_stride is None else out_stride,
                                                count if audio_stride is None else audio_stride,
                                                count if sc_stride is None else sc_stride, _stream(stream)))

    def close(self):
        if self.handle:
            lib.mi_limiter_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _dynproc_dict(p):
    """Entries [0, count) of the three tables, float32."""
    return {"hold": p.hold,
            "attack": [{"level": np.float32(r.level), "tau": np.float32(r.tau)} for r in p.attack[:p.attacks]],
            "release": [{"level": np.float32(r.level), "tau": np.float32(r.tau)} for r in p.release[:p.releases]],
            "splines": [dict([(n, np.float32(getattr(s, n))) for n in ("pre_ratio", "post_ratio", "knee_start", "knee_stop",
                                                                       "thresh", "makeup")] +
                             [("herm", np.array(s.herm[:], np.float32))]) for s in p.spline[:p.splines]]}


class DynamicProcessorBank(_DynamicsBank):
    """`channels` x lsp::dspu::DynamicProcessor (mi_dynproc_bank_*): envelope follower whose attack and release times depend
    on the level of the envelope, and a gain curve through up to four dots with a knee each; every channel with settings of
    its own.  A fresh channel has four dots at (0, 0, 0) that cannot be evaluated: configure() sets all of them."""
    UNIT = "dynproc"
    DOTS, RANGES = 4, 5
    set_timings = None                      # the reference has none: times are per range, set_attack_time / set_release_time

    @staticmethod
    def _settings(sample_rate=0, hold=0.0, in_ratio=1.0, out_ratio=1.0, dots=(), attack_levels=(), release_levels=(),
                  attack_times=(0.0,), release_times=(0.0,)):
        """dots: up to four (input, output, knee) or None (off); levels: up to four, None or negative is off; times: up to
        five in ms, [0] the default, [i + 1] from level i on.  What is not given is off (dots, levels) or 0 (times)."""
        from .capi import DynprocDot, DynprocSettings
        pad = lambda v, n, fill: [fill if x is None else x for x in list(v)] + [fill] * (n - len(v))
        s = DynprocSettings(sample_rate, hold, in_ratio, out_ratio)
        for i, d in enumerate(pad(dots, 4, (-1.0, -1.0, -1.0))):
            s.dot[i] = DynprocDot(*d)
        s.attack_level[:] = pad(attack_levels, 4, -1.0)
        s.release_level[:] = pad(release_levels, 4, -1.0)
        s.attack_time[:] = pad(attack_times, 5, 0.0)
        s.release_time[:] = pad(release_times, 5, 0.0)
        return s

    @classmethod
    def compute_params(cls, **settings):
        """update_settings() of one processor on the host (mi_dynproc_compute_params): no device needed.  Keywords as
        configure()."""
        from .capi import DynprocParams
        s, p = cls._settings(**settings), DynprocParams()
        check(lib.mi_dynproc_compute_params(byref(s), byref(p)))
        return _dynproc_dict(p)

    def set_in_ratio(self, channel, ratio):
        check(lib.mi_dynproc_bank_set_in_ratio(self.handle, channel, ratio))

    def set_out_ratio(self, channel, ratio):
        check(lib.mi_dynproc_bank_set_out_ratio(self.handle, channel, ratio))

    def set_dot(self, channel, id, dot):
        """dot: (input, output, knee), or None to switch it off."""
        from .capi import DynprocDot
        check(lib.mi_dynproc_bank_set_dot(self.handle, channel, id, None if dot is None else byref(DynprocDot(*dot))))

    def set_attack_level(self, channel, id, level):
        check(lib.mi_dynproc_bank_set_attack_level(self.handle, channel, id, level))

    def set_release_level(self, channel, id, level):
        check(lib.mi_dynproc_bank_set_release_level(self.handle, channel, id, level))

    def set_attack_time(self, channel, id, time):
        check(lib.mi_dynproc_bank_set_attack_time(self.handle, channel, id, time))

    def set_release_time(self, channel, id, time):
        check(lib.mi_dynproc_bank_set_release_time(self.handle, channel, id, time))

    def configure(self, channel, **settings):
        """Every setter of one channel; keywords as _settings()."""
        s = self._settings(**settings)
        self.set_sample_rate(channel, s.sample_rate)
        self.set_hold(channel, s.hold)
        self.set_in_ratio(channel, s.in_ratio)
        self.set_out_ratio(channel, s.out_ratio)
        for i in range(self.DOTS):
            d = s.dot[i]
            self.set_dot(channel, i, None if d.input < 0 and d.output < 0 and d.knee < 0 else (d.input, d.output, d.knee))
            self.set_attack_level(channel, i, s.attack_level[i])
            self.set_release_level(channel, i, s.release_level[i])
        for i in range(self.RANGES):
            self.set_attack_time(channel, i, s.attack_time[i])
            self.set_release_time(channel, i, s.release_time[i])

    def get_params(self, channel):
        from .capi import DynprocParams
        p = DynprocParams()
        check(lib.mi_dynproc_bank_get_params(self.handle, channel, byref(p)))
        return _dynproc_dict(p)

    def get_state(self, channel, stream=None):
        """(fEnvelope, fPeak, nHoldCounter) of the channel; the envelope and the peak as numpy float32."""
        e, p, h = c_float(), c_float(), c_uint32()
        check(lib.mi_dynproc_bank_get_state(self.handle, channel, byref(e), byref(p), byref(h), _stream(stream)))
        return np.float32(e.value), np.float32(p.value), h.value

    def curve(self, out, inp, dots, out_stride=None, in_stride=None, stream=None):
        """curve(out, in, dots) of every channel: out = gain(|in|) |in|."""
        check(lib.mi_dynproc_bank_curve(self.handle, _ptr(out), _ptr(inp), dots, dots if out_stride is None else out_stride,
                                        dots if in_stride is None else in_stride, _stream(stream)))

    def model(self, out, inp, dots, out_stride=None, in_stride=None, stream=None):
        """model(out, in, dots) of every channel: the curve without its knees."""
        check(lib.mi_dynproc_bank_model(self.handle, _ptr(out), _ptr(inp), dots, dots if out_stride is None else out_stride,
                                        dots if in_stride is None else in_stride, _stream(stream)))


def _autogain_dict(p):
    curve = lambda c: dict((n, np.float32(getattr(c, n))) for n in ("x1", "x2", "t", "a", "b", "c", "d"))
    d = dict((n, np.float32(getattr(p, n))) for n in ("short_kgrow", "short_kfall", "long_kgrow", "long_kfall", "silence",
                                                      "deviation", "max_gain"))
    d.update(short_comp=curve(p.short_comp), out_comp=curve(p.out_comp), flags=p.flags)
    return d


def _n(count, stride):
    return count if stride is None else stride


class AutoGainBank:
    """`channels` x lsp::dspu::AutoGain (mi_autogain_bank_*): a long-period and a short-period loudness and the expected
    level in, one VCA gain per sample out; every channel with settings of its own."""
    F_QUICK_AMP, F_MAX_GAIN, F_SURGE_UP, F_SURGE_DOWN = 2, 4, 8, 16

    def __init__(self, channels):
        h = c_void_p()
        check(lib.mi_autogain_bank_create(byref(h), channels))
        self.handle, self.channels = h, channels

    @staticmethod
    def compute_params(sample_rate=0, flags=0, short_grow=0.0, short_fall=0.0, long_grow=0.0, long_fall=0.0, silence=2.5119e-4,
                       deviation=1.99526, max_gain=3.98107):
        """update() of one unit on the host (mi_autogain_compute_params): no device needed."""
        from .capi import AutoGainParams, AutoGainSettings
        s = AutoGainSettings(sample_rate, flags, short_grow, short_fall, long_grow, long_fall, silence, deviation, max_gain)
        p = AutoGainParams()
        check(lib.mi_autogain_compute_params(byref(s), byref(p)))
        return _autogain_dict(p)

    def set_sample_rate(self, channel, sr):
        check(lib.mi_autogain_bank_set_sample_rate(self.handle, channel, sr))

    def set_silence_threshold(self, channel, threshold):
        check(lib.mi_autogain_bank_set_silence_threshold(self.handle, channel, threshold))

    def set_deviation(self, channel, deviation):
        check(lib.mi_autogain_bank_set_deviation(self.handle, channel, deviation))

    def set_short_grow(self, channel, value):
        check(lib.mi_autogain_bank_set_short_grow(self.handle, channel, value))

    def set_short_fall(self, channel, value):
        check(lib.mi_autogain_bank_set_short_fall(self.handle, channel, value))

    def set_short_speed(self, channel, grow, fall):
        check(lib.mi_autogain_bank_set_short_speed(self.handle, channel, grow, fall))

    def set_long_grow(self, channel, value):
        check(lib.mi_autogain_bank_set_long_grow(self.handle, channel, value))

    def set_long_fall(self, channel, value):
        check(lib.mi_autogain_bank_set_long_fall(self.handle, channel, value))

    def set_long_speed(self, channel, grow, fall):
        check(lib.mi_autogain_bank_set_long_speed(self.handle, channel, grow, fall))

    def set_max_gain(self, channel, value, enable=None):
        """set_max_gain(value) or, with enable, set_max_gain(value, enable)."""
        if enable is None:
            check(lib.mi_autogain_bank_set_max_gain(self.handle, channel, value))
        else:
            check(lib.mi_autogain_bank_set_max_gain_control(self.handle, channel, value, int(bool(enable))))

    def enable_max_gain(self, channel, enable):
        check(lib.mi_autogain_bank_enable_max_gain(self.handle, channel, int(bool(enable))))

    def enable_quick_amplifier(self, channel, enable):
        check(lib.mi_autogain_bank_enable_quick_amplifier(self.handle, channel, int(bool(enable))))

    def configure(self, channel, sample_rate, short_grow, short_fall, long_grow, long_fall, silence, deviation, max_gain,
                  quick_amp=False, limit=False):
        """Every setter of one channel."""
        self.set_sample_rate(channel, sample_rate)
        self.set_short_speed(channel, short_grow, short_fall)
        self.set_long_speed(channel, long_grow, long_fall)
        self.set_silence_threshold(channel, silence)
        self.set_deviation(channel, deviation)
        self.set_max_gain(channel, max_gain, limit)
        self.enable_quick_amplifier(channel, quick_amp)

    def update_settings(self, stream=None):
        check(lib.mi_autogain_bank_update_settings(self.handle, _stream(stream)))

    def get_params(self, channel):
        from .capi import AutoGainParams
        p = AutoGainParams()
        check(lib.mi_autogain_bank_get_params(self.handle, channel, byref(p)))
        return _autogain_dict(p)

    def get_state(self, channel, stream=None):
        """(fCurrGain, fOutGain, nFlags without F_UPDATE) of the channel; the gains as numpy float32."""
        g, o, f = c_float(), c_float(), c_uint32()
        check(lib.mi_autogain_bank_get_state(self.handle, channel, byref(g), byref(o), byref(f), _stream(stream)))
        return np.float32(g.value), np.float32(o.value), f.value

    def process(self, vca, llong, lshort, lexp, count, vca_stride=None, long_stride=None, short_stride=None, exp_stride=None,
                stream=None):
        """process(vca, llong, lshort, lexp, count); vca may be any of the inputs (in place)."""
        check(lib.mi_autogain_bank_process(self.handle, _ptr(vca), _ptr(llong), _ptr(lshort), _ptr(lexp), count, _n(count, vca_stride),
                                           _n(count, long_stride), _n(count, short_stride), _n(count, exp_stride), _stream(stream)))

    def process_level(self, vca, llong, lshort, levels, count, vca_stride=None, long_stride=None, short_stride=None, stream=None):
        """process(vca, llong, lshort, float lexp, count) with levels[channels] in device memory."""
        check(lib.mi_autogain_bank_process_level(self.handle, _ptr(vca), _ptr(llong), _ptr(lshort), _ptr(levels), count,
                                                 _n(count, vca_stride), _n(count, long_stride), _n(count, short_stride),
                                                 _stream(stream)))

    def process_apply(self, out, audio, llong, lshort, lexp, count, out_stride=None, audio_stride=None, long_stride=None,
                      short_stride=None, exp_stride=None, stream=None):
        """out = audio * vca in one launch; out may be audio or any of the level rows."""
        check(lib.mi_autogain_bank_process_apply(self.handle, _ptr(out), _ptr(audio), _ptr(llong), _ptr(lshort), _ptr(lexp), count,
                                                 _n(count, out_stride), _n(count, audio_stride), _n(count, long_stride),
                                                 _n(count, short_stride), _n(count, exp_stride), _stream(stream)))

    def close(self):
        if self.handle:
            lib.mi_autogain_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SimpleAutoGainBank:
    """`channels` x lsp::dspu::SimpleAutoGain (mi_simple_autogain_bank_*): the gain grows below a threshold, falls above it
    and stays within [min, max]; every channel with settings of its own."""

    def __init__(self, channels):
        h = c_void_p()
        check(lib.mi_simple_autogain_bank_create(byref(h), channels))
        self.handle, self.channels = h, channels

    @staticmethod
    def _dict(p):
        return dict((n, np.float32(getattr(p, n))) for n in ("kgrow", "kfall", "threshold", "min_gain", "max_gain"))

    @staticmethod
    def compute_params(sample_rate=0, grow=0.0, fall=0.0, threshold=0.0, min_gain=0.000001, max_gain=1.0):
        """update() of one unit on the host (mi_simple_autogain_compute_params): no device needed."""
        from .capi import SimpleAutoGainParams, SimpleAutoGainSettings
        s = SimpleAutoGainSettings(sample_rate, grow, fall, threshold, min_gain, max_gain)
        p = SimpleAutoGainParams()
        check(lib.mi_simple_autogain_compute_params(byref(s), byref(p)))
        return SimpleAutoGainBank._dict(p)

    def set_sample_rate(self, channel, sr):
        check(lib.mi_simple_autogain_bank_set_sample_rate(self.handle, channel, sr))

    def set_grow(self, channel, value):
        check(lib.mi_simple_autogain_bank_set_grow(self.handle, channel, value))

    def set_fall(self, channel, value):
        check(lib.mi_simple_autogain_bank_set_fall(self.handle, channel, value))

    def set_speed(self, channel, grow, fall):
        check(lib.mi_simple_autogain_bank_set_speed(self.handle, channel, grow, fall))

    def set_max_gain(self, channel, value):
        check(lib.mi_simple_autogain_bank_set_max_gain(self.handle, channel, value))

    def set_min_gain(self, channel, value):
        check(lib.mi_simple_autogain_bank_set_min_gain(self.handle, channel, value))

    def set_gain(self, channel, lo, hi):
        check(lib.mi_simple_autogain_bank_set_gain(self.handle, channel, lo, hi))

    def set_threshold(self, channel, threshold):
        check(lib.mi_simple_autogain_bank_set_threshold(self.handle, channel, threshold))

    def update_settings(self, stream=None):
        check(lib.mi_simple_autogain_bank_update_settings(self.handle, _stream(stream)))

    def get_params(self, channel):
        from .capi import SimpleAutoGainParams
        p = SimpleAutoGainParams()
        check(lib.mi_simple_autogain_bank_get_params(self.handle, channel, byref(p)))
        return self._dict(p)

    def get_state(self, channel, stream=None):
        """fCurrGain of the channel as numpy float32."""
        g = c_float()
        check(lib.mi_simple_autogain_bank_get_state(self.handle, channel, byref(g), _stream(stream)))
        return np.float32(g.value)

    def process(self, out, inp, count, out_stride=None, in_stride=None, stream=None):
        """process(dst, src, count); out may be inp (in place)."""
        check(lib.mi_simple_autogain_bank_process(self.handle, _ptr(out), _ptr(inp), count, _n(count, out_stride),
                                                  _n(count, in_stride), _stream(stream)))

    def close(self):
        if self.handle:
            lib.mi_simple_autogain_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _sidechain_dict(p):
    return {"reactivity": p.reactivity, "tau": np.float32(p.tau), "interval": np.float32(p.interval), "capacity": p.capacity,
            "mode": p.mode, "source": p.source, "flags": p.flags, "gain": np.float32(p.gain)}


class SidechainBank:
    """`channels` x lsp::dspu::Sidechain (mi_sidechain_bank_*): source selection, pre-amplification and the peak / RMS /
    low-pass / uniform detectors, every channel with settings of its own."""
    SCS_MIDDLE, SCS_SIDE, SCS_LEFT, SCS_RIGHT, SCS_AMIN, SCS_AMAX = range(6)
    SCM_PEAK, SCM_RMS, SCM_LPF, SCM_UNIFORM = range(4)
    SCSM_STEREO, SCSM_MIDSIDE = range(2)
    SCF_MIDSIDE, SCF_UPDATE, SCF_CLEAR = 1, 2, 4
    ALL = 0xFFFFFFFF

    def __init__(self, channels, inputs=1, max_reactivity_ms=50.0):
        h = c_void_p()
        check(lib.mi_sidechain_bank_create(byref(h), channels, inputs, float(max_reactivity_ms)))
        self.handle, self.channels, self.inputs = h, channels, inputs

    @staticmethod
    def compute_params(sample_rate, max_reactivity, reactivity):
        """update_settings() and the ring's capacity of one sidechain on the host (mi_sidechain_compute_params): no device needed."""
        from .capi import SidechainParams
        p = SidechainParams()
        check(lib.mi_sidechain_compute_params(sample_rate, float(max_reactivity), float(reactivity), byref(p)))
        return _sidechain_dict(p)

    def set_sample_rate(self, channel, sr):
        check(lib.mi_sidechain_bank_set_sample_rate(self.handle, channel, sr))

    def set_reactivity(self, channel, reactivity):
        check(lib.mi_sidechain_bank_set_reactivity(self.handle, channel, float(reactivity)))

    def set_stereo_mode(self, channel, mode):
        check(lib.mi_sidechain_bank_set_stereo_mode(self.handle, channel, mode))

    def set_source(self, channel, source):
        check(lib.mi_sidechain_bank_set_source(self.handle, channel, source))

    def set_mode(self, channel, mode):
        check(lib.mi_sidechain_bank_set_mode(self.handle, channel, mode))

    def set_gain(self, channel, gain):
        check(lib.mi_sidechain_bank_set_gain(self.handle, channel, float(gain)))

    def configure(self, channel, sample_rate, reactivity, mode, source=0, stereo_mode=0, gain=1.0):
        """Every setter of one channel."""
        self.set_sample_rate(channel, sample_rate)
        self.set_reactivity(channel, reactivity)
        self.set_mode(channel, mode)
        self.set_source(channel, source)
        self.set_stereo_mode(channel, stereo_mode)
        self.set_gain(channel, gain)

    def clear(self, channel=ALL):
        check(lib.mi_sidechain_bank_clear(self.handle, channel))

    def update_settings(self, stream=None):
        check(lib.mi_sidechain_bank_update_settings(self.handle, _stream(stream)))

    def get_params(self, channel):
        from .capi import SidechainParams
        p = SidechainParams()
        check(lib.mi_sidechain_bank_get_params(self.handle, channel, byref(p)))
        return _sidechain_dict(p)

    def get_state(self, channel, stream=None):
        """(fRmsValue as numpy float32, nRefresh, the ring position) of the channel."""
        v, r, h = c_float(), c_uint32(), c_uint32()
        check(lib.mi_sidechain_bank_get_state(self.handle, channel, byref(v), byref(r), byref(h), _stream(stream)))
        return np.float32(v.value), r.value, h.value

    def process(self, out, in0, in1, count, out_stride=None, in0_stride=None, in1_stride=None, stream=None):
        """process(out, in, samples): in1 None for one input, in0 None for silence; out may be an input (in place)."""
        check(lib.mi_sidechain_bank_process(self.handle, _ptr(out), None if in0 is None else _ptr(in0), None if in1 is None else _ptr(in1),
                                            count, count if out_stride is None else out_stride,
                                            count if in0_stride is None else in0_stride,
                                            count if in1_stride is None else in1_stride, _stream(stream)))

    def premix(self, out, in0, in1, count, out_stride=None, in0_stride=None, in1_stride=None, stream=None):
        """The signed selected source, before magnitude and gain."""
        check(lib.mi_sidechain_bank_premix(self.handle, _ptr(out), None if in0 is None else _ptr(in0), None if in1 is None else _ptr(in1),
                                           count, count if out_stride is None else out_stride,
                                           count if in0_stride is None else in0_stride,
                                           count if in1_stride is None else in1_stride, _stream(stream)))

    def process_premixed(self, out, inp, count, out_stride=None, in_stride=None, stream=None):
        """Magnitude, gain, ring and detector on rows that premix() wrote."""
        check(lib.mi_sidechain_bank_process_premixed(self.handle, _ptr(out), _ptr(inp), count, count if out_stride is None else out_stride,
                                                     count if in_stride is None else in_stride, _stream(stream)))

    def close(self):
        if self.handle:
            lib.mi_sidechain_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _StereoMeterBank:
    """What CorrelometerBank and PanometerBank share: two input rows per channel, sliding-window sums over per-channel rings on
    the device, a period per channel."""
    ALL = 0xFFFFFFFF
    _name = None

    def _fn(self, what):
        return getattr(lib, "mi_%s_bank_%s" % (self._name, what))

    def __init__(self, channels, max_period):
        h = c_void_p()
        check(getattr(lib, "mi_%s_bank_create" % self._name)(byref(h), channels, max_period))
        self.handle, self.channels, self.max_period = h, channels, max_period

    def set_period(self, channel, period):
        check(self._fn("set_period")(self.handle, channel, period))

    def clear(self, channel=ALL):
        check(self._fn("clear")(self.handle, channel))

    def update_settings(self, stream=None):
        check(self._fn("update_settings")(self.handle, _stream(stream)))

    def process(self, out, a, b, count, out_stride=None, a_stride=None, b_stride=None, stream=None):
        """process(dst, a, b, count); out may be a or b (in place)."""
        check(self._fn("process")(self.handle, _ptr(out), _ptr(a), _ptr(b), count, count if out_stride is None else out_stride,
                                  count if a_stride is None else a_stride, count if b_stride is None else b_stride, _stream(stream)))

    def close(self):
        if self.handle:
            self._fn("destroy")(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CorrelometerBank(_StereoMeterBank):
    """`channels` x lsp::dspu::Correlometer (mi_correlometer_bank_*): the normalised correlation of two rows over a sliding
    window, every channel with a period of its own."""
    _name = "correlometer"

    def configure(self, channel, period):
        """Every setter of one channel."""
        self.set_period(channel, period)

    def get_params(self, channel):
        from .capi import CorrelometerParams
        p = CorrelometerParams()
        check(lib.mi_correlometer_bank_get_params(self.handle, channel, byref(p)))
        return {"period": p.period, "capacity": p.capacity, "max_period": p.max_period}

    def get_state(self, channel, stream=None):
        """sCorr's v, a, b as numpy float32, nHead and nWindow of the channel."""
        from .capi import CorrelometerState
        s = CorrelometerState()
        check(lib.mi_correlometer_bank_get_state(self.handle, channel, byref(s), _stream(stream)))
        return {"v": np.float32(s.v), "a": np.float32(s.a), "b": np.float32(s.b), "head": s.head, "window": s.window}

    def set_state(self, channel, v, a, b, head, window, zero_rings=False, stream=None):
        from .capi import CorrelometerState
        s = CorrelometerState(float(v), float(a), float(b), head, window)
        check(lib.mi_correlometer_bank_set_state(self.handle, channel, byref(s), 1 if zero_rings else 0, _stream(stream)))


class PanometerBank(_StereoMeterBank):
    """`channels` x lsp::dspu::Panometer (mi_panometer_bank_*): the balance of two rows out of the window sums of their squares,
    linear or equal-power law, every channel with settings of its own."""
    _name = "panometer"
    PAN_LAW_LINEAR, PAN_LAW_EQUAL_POWER = range(2)

    def set_pan_law(self, channel, law):
        check(lib.mi_panometer_bank_set_pan_law(self.handle, channel, law))

    def set_default_pan(self, channel, default_pan):
        check(lib.mi_panometer_bank_set_default_pan(self.handle, channel, float(default_pan)))

    def configure(self, channel, period, law=PAN_LAW_EQUAL_POWER, default_pan=0.5):
        """Every setter of one channel."""
        self.set_period(channel, period)
        self.set_pan_law(channel, law)
        self.set_default_pan(channel, default_pan)

    def get_params(self, channel):
        from .capi import PanometerParams
        p = PanometerParams()
        check(lib.mi_panometer_bank_get_params(self.handle, channel, byref(p)))
        return {"period": p.period, "capacity": p.capacity, "max_period": p.max_period, "law": p.law, "norm": np.float32(p.norm),
                "default_pan": np.float32(p.default_pan)}

    def get_state(self, channel, stream=None):
        """fValueA and fValueB as numpy float32, nHead and nWindow of the channel."""
        from .capi import PanometerState
        s = PanometerState()
        check(lib.mi_panometer_bank_get_state(self.handle, channel, byref(s), _stream(stream)))
        return {"value_a": np.float32(s.value_a), "value_b": np.float32(s.value_b), "head": s.head, "window": s.window}

    def set_state(self, channel, value_a, value_b, head, window, zero_rings=False, stream=None):
        from .capi import PanometerState
        s = PanometerState(float(value_a), float(value_b), head, window)
        check(lib.mi_panometer_bank_set_state(self.handle, channel, byref(s), 1 if zero_rings else 0, _stream(stream)))


def _opt(x):
    return None if x is None else _ptr(x)


class PeakMeterBank:
    """`channels` x lsp::dspu::PeakMeter (mi_peakmeter_bank_*): a peak hold/decay follower per channel, fPeak and nCounter on the
    device."""
    ALL = 0xFFFFFFFF

    def __init__(self, channels):
        h = c_void_p()
        check(lib.mi_peakmeter_bank_create(byref(h), channels))
        self.handle, self.channels = h, channels

    def set_sample_rate(self, channel, sample_rate):
        check(lib.mi_peakmeter_bank_set_sample_rate(self.handle, channel, sample_rate))

    def set_hold_time(self, channel, hold):
        check(lib.mi_peakmeter_bank_set_hold_time(self.handle, channel, float(hold)))

    def set_release_time(self, channel, release):
        check(lib.mi_peakmeter_bank_set_release_time(self.handle, channel, float(release)))

    def set_time(self, channel, hold, release):
        check(lib.mi_peakmeter_bank_set_time(self.handle, channel, float(hold), float(release)))

    def configure(self, channel, sample_rate, hold, release):
        """Every setter of one channel (times in milliseconds)."""
        self.set_sample_rate(channel, sample_rate)
        self.set_time(channel, hold, release)

    def clear(self, channel=ALL):
        check(lib.mi_peakmeter_bank_clear(self.handle, channel))

    def update_settings(self, stream=None):
        check(lib.mi_peakmeter_bank_update_settings(self.handle, _stream(stream)))

    def get_params(self, channel):
        """fTau as numpy float32 and nHold as update_settings() computes them."""
        from .capi import PeakMeterParams
        p = PeakMeterParams()
        check(lib.mi_peakmeter_bank_get_params(self.handle, channel, byref(p)))
        return {"tau": np.float32(p.tau), "hold": p.hold, "factor": np.float32(p.factor), "count": p.count}

    def set_params(self, channel, tau, hold):
        from .capi import PeakMeterParams
        p = PeakMeterParams(float(tau), hold, 0.0, 0)
        check(lib.mi_peakmeter_bank_set_params(self.handle, channel, byref(p)))

    def get_state(self, channel, stream=None):
        from .capi import PeakMeterState
        s = PeakMeterState()
        check(lib.mi_peakmeter_bank_get_state(self.handle, channel, byref(s), _stream(stream)))
        return {"peak": np.float32(s.peak), "counter": s.counter}

    def set_state(self, channel, peak, counter, stream=None):
        from .capi import PeakMeterState
        s = PeakMeterState(float(peak), counter)
        check(lib.mi_peakmeter_bank_set_state(self.handle, channel, byref(s), _stream(stream)))

    def process(self, dst, src, count, peaks=None, dst_stride=None, src_stride=None, stream=None):
        """process(dst, src, count); dst None: the state only; dst may be src.  peaks: a device array of `channels` floats for the
        peak after the last sample, or None."""
        check(lib.mi_peakmeter_bank_process(self.handle, _opt(dst), _opt(src), _opt(peaks), count,
                                            count if dst_stride is None else dst_stride,
                                            count if src_stride is None else src_stride, _stream(stream)))

    def process_value(self, peaks, values, count, stream=None):
        """process(value, count) of every channel: values and peaks are device arrays of `channels` floats (peaks may be None)."""
        check(lib.mi_peakmeter_bank_process_value(self.handle, _opt(peaks), _opt(values), count, _stream(stream)))

    def close(self):
        if self.handle:
            lib.mi_peakmeter_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MeterGraphBank:
    """`channels` x lsp::dspu::MeterGraph (mi_metergraph_bank_*): full-rate rows decimated into rings of display frames on the
    device.  Methods: ABS_MAXIMUM .. PEAK as meter_method_t has them."""
    ALL = 0xFFFFFFFF
    ABS_MAXIMUM, ABS_MINIMUM, SIGN_MAXIMUM, SIGN_MINIMUM, PEAK = range(5)

    def __init__(self, channels, max_frames):
        h = c_void_p()
        check(lib.mi_metergraph_bank_create(byref(h), channels, max_frames))
        self.handle, self.channels, self.max_frames = h, channels, max_frames

    def init(self, channel, frames, period, default_value=0.0):
        check(lib.mi_metergraph_bank_init(self.handle, channel, frames, period, float(default_value)))

    def set_method(self, channel, method):
        check(lib.mi_metergraph_bank_set_method(self.handle, channel, method))

    def set_period(self, channel, period):
        check(lib.mi_metergraph_bank_set_period(self.handle, channel, period))

    def set_default_value(self, channel, value):
        check(lib.mi_metergraph_bank_set_default_value(self.handle, channel, float(value)))

    def fill(self, level, channel=ALL):
        check(lib.mi_metergraph_bank_fill(self.handle, channel, float(level)))

    def clear(self, channel=ALL):
        check(lib.mi_metergraph_bank_clear(self.handle, channel))

    def update_settings(self, stream=None):
        check(lib.mi_metergraph_bank_update_settings(self.handle, _stream(stream)))

    def get_params(self, channel):
        from .capi import MeterGraphParams
        p = MeterGraphParams()
        check(lib.mi_metergraph_bank_get_params(self.handle, channel, byref(p)))
        return {"method": p.method, "period": p.period, "frames": p.frames, "default_value": np.float32(p.default_value)}

    def get_state(self, channel, stream=None):
        """fCurrent, nCount, nHead and the ring's words in storage order."""
        from .capi import MeterGraphState
        s = MeterGraphState()
        ring = np.zeros(max(1, self.get_params(channel)["frames"]), np.float32)
        check(lib.mi_metergraph_bank_get_state(self.handle, channel, byref(s), ring.ctypes.data_as(c_void_p), _stream(stream)))
        return {"current": np.float32(s.current), "count": s.count, "head": s.head, "ring": ring[:self.get_params(channel)["frames"]]}

    def set_state(self, channel, current, count, head, ring=None, stream=None):
        from .capi import MeterGraphState
        s = MeterGraphState(float(current), count, head)
        r = None if ring is None else np.ascontiguousarray(ring, np.float32)
        check(lib.mi_metergraph_bank_set_state(self.handle, channel, byref(s), None if r is None else r.ctypes.data_as(c_void_p), _stream(stream)))

    def process(self, src, count, gains=None, stride=None, stream=None):
        """process(s, n) of every channel, or process(s, gain, n) with gains a device array of `channels` floats."""
        check(lib.mi_metergraph_bank_process(self.handle, _opt(src), _opt(gains), count, count if stride is None else stride, _stream(stream)))

    def process_value(self, values, stream=None):
        """process(sample) of every channel: values is a device array of `channels` floats."""
        check(lib.mi_metergraph_bank_process_value(self.handle, _opt(values), _stream(stream)))

    def read(self, dst, count, stride=None, stream=None):
        check(lib.mi_metergraph_bank_read(self.handle, _opt(dst), count, count if stride is None else stride, _stream(stream)))

    def level(self, levels, stream=None):
        check(lib.mi_metergraph_bank_level(self.handle, _opt(levels), _stream(stream)))

    def close(self):
        if self.handle:
            lib.mi_metergraph_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ScaledMeterGraphBank:
    """`channels` x lsp::dspu::ScaledMeterGraph (mi_scaled_metergraph_bank_*): full-rate rows sampled into a history of sub-samples
    and into a ring of display frames whose period can change; a new period re-decimates the history.  Methods as MeterGraphBank's."""
    ALL = 0xFFFFFFFF
    ABS_MAXIMUM, ABS_MINIMUM, SIGN_MAXIMUM, SIGN_MINIMUM, PEAK = range(5)
    FRAMES_GAP = 16

    def __init__(self, channels, max_frames, max_subframes):
        h = c_void_p()
        check(lib.mi_scaled_metergraph_bank_create(byref(h), channels, max_frames, max_subframes))
        self.handle, self.channels, self.max_frames, self.max_subframes = h, channels, max_frames, max_subframes

    def init(self, channel, frames, subsampling, max_period):
        check(lib.mi_scaled_metergraph_bank_init(self.handle, channel, frames, subsampling, max_period))

    def set_method(self, channel, method):
        check(lib.mi_scaled_metergraph_bank_set_method(self.handle, channel, method))

    def set_period(self, channel, period):
        check(lib.mi_scaled_metergraph_bank_set_period(self.handle, channel, period))

    def fill(self, level, channel=ALL):
        check(lib.mi_scaled_metergraph_bank_fill(self.handle, channel, float(level)))

    def update_settings(self, stream=None):
        check(lib.mi_scaled_metergraph_bank_update_settings(self.handle, _stream(stream)))

    def get_params(self, channel):
        from .capi import ScaledMeterGraphParams
        p = ScaledMeterGraphParams()
        check(lib.mi_scaled_metergraph_bank_get_params(self.handle, channel, byref(p)))
        return {n: getattr(p, n) for n, _ in ScaledMeterGraphParams._fields_}

    def get_state(self, channel, stream=None):
        """Both samplers' words (mi_scaled_metergraph_state_t's names) and both rings in storage order: "history", "ring"."""
        from .capi import ScaledMeterGraphState
        s = ScaledMeterGraphState()
        p = self.get_params(channel)
        rings = p["frames"] != 0
        history = np.zeros(p["subframes"] + self.FRAMES_GAP if rings else 1, np.float32)
        ring = np.zeros(p["frames"] + self.FRAMES_GAP if rings else 1, np.float32)
        check(lib.mi_scaled_metergraph_bank_get_state(self.handle, channel, byref(s), history.ctypes.data_as(c_void_p), ring.ctypes.data_as(c_void_p),
                                                      _stream(stream)))
        out = {n: getattr(s, n) for n, _ in ScaledMeterGraphState._fields_}
        out["history_current"], out["frames_current"] = np.float32(s.history_current), np.float32(s.frames_current)
        out["history"], out["ring"] = (history, ring) if rings else (history[:0], ring[:0])
        return out

    def set_state(self, channel, state, history=None, ring=None, stream=None):
        """state: a dict with mi_scaled_metergraph_state_t's names; history and ring: host arrays in storage order, or None."""
        from .capi import ScaledMeterGraphState
        s = ScaledMeterGraphState(*[(float if n.endswith("current") else int)(state[n]) for n, _ in ScaledMeterGraphState._fields_])
        h = None if history is None else np.ascontiguousarray(history, np.float32)
        r = None if ring is None else np.ascontiguousarray(ring, np.float32)
        check(lib.mi_scaled_metergraph_bank_set_state(self.handle, channel, byref(s), None if h is None else h.ctypes.data_as(c_void_p),
                                                      None if r is None else r.ctypes.data_as(c_void_p), _stream(stream)))

    def process(self, src, count, gains=None, stride=None, stream=None):
        """process(s, n) of every channel, or process(s, gain, n) with gains a device array of `channels` floats."""
        check(lib.mi_scaled_metergraph_bank_process(self.handle, _opt(src), _opt(gains), count, count if stride is None else stride, _stream(stream)))

    def process_value(self, values, stream=None):
        """process(sample) of every channel: values is a device array of `channels` floats."""
        check(lib.mi_scaled_metergraph_bank_process_value(self.handle, _opt(values), _stream(stream)))

    def read(self, dst, count, stride=None, stream=None):
        check(lib.mi_scaled_metergraph_bank_read(self.handle, _opt(dst), count, count if stride is None else stride, _stream(stream)))

    def level(self, levels, stream=None):
        check(lib.mi_scaled_metergraph_bank_level(self.handle, _opt(levels), _stream(stream)))

    def close(self):
        if self.handle:
            lib.mi_scaled_metergraph_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class QuantizedCounterBank:
    """`channels` x lsp::dspu::QuantizedCounter (mi_qcounter_bank_*): the histogram of the last `period` samples of every row over
    `levels` quantisation levels of [min, max), with a counter for what lies below the range and one for above, on the device."""
    ALL = 0xFFFFFFFF

    def __init__(self, channels, max_period, max_levels):
        h = c_void_p()
        check(lib.mi_qcounter_bank_create(byref(h), channels, max_period, max_levels))
        self.handle, self.channels, self.max_period, self.max_levels = h, channels, max_period, max_levels

    def set_period(self, channel, period):
        check(lib.mi_qcounter_bank_set_period(self.handle, channel, period))

    def set_levels(self, channel, levels):
        check(lib.mi_qcounter_bank_set_levels(self.handle, channel, levels))

    def set_min_value(self, channel, value):
        check(lib.mi_qcounter_bank_set_min_value(self.handle, channel, float(value)))

    def set_max_value(self, channel, value):
        check(lib.mi_qcounter_bank_set_max_value(self.handle, channel, float(value)))

    def set_value_range(self, channel, min_value, max_value):
        check(lib.mi_qcounter_bank_set_value_range(self.handle, channel, float(min_value), float(max_value)))

    def set_range(self, channel, min_value, max_value, levels):
        check(lib.mi_qcounter_bank_set_range(self.handle, channel, float(min_value), float(max_value), levels))

    def needs_update(self, channel):
        v = ctypes.c_int()
        check(lib.mi_qcounter_bank_needs_update(self.handle, channel, byref(v)))
        return bool(v.value)

    def update_settings(self, stream=None):
        check(lib.mi_qcounter_bank_update_settings(self.handle, _stream(stream)))

    def clear(self, channel=ALL):
        check(lib.mi_qcounter_bank_clear(self.handle, channel))

    def process(self, src, count, stride=None, stream=None):
        check(lib.mi_qcounter_bank_process(self.handle, _opt(src), count, count if stride is None else stride, _stream(stream)))

    def read(self, counters, stride, stream=None):
        """counters: a device array [channels, stride] of uint32: the bins of the largest `levels`, then below, then above."""
        check(lib.mi_qcounter_bank_read(self.handle, _opt(counters), stride, _stream(stream)))

    def set_wave_combining(self, on):
        check(lib.mi_qcounter_bank_set_wave_combining(self.handle, int(bool(on))))

    def get_params(self, channel):
        from .capi import QuantizedCounterParams
        p = QuantizedCounterParams()
        check(lib.mi_qcounter_bank_get_params(self.handle, channel, byref(p)))
        return {"period": p.period, "levels": p.levels, "min_value": np.float32(p.min_value), "max_value": np.float32(p.max_value),
                "rstep": np.float32(p.rstep), "update": bool(p.update)}

    def get_state(self, channel, stream=None):
        """nHead, nCount, nCapacity, the ring's words in storage order and vCounters' max_levels + 2 words."""
        from .capi import QuantizedCounterState
        s = QuantizedCounterState()
        check(lib.mi_qcounter_bank_get_state(self.handle, channel, byref(s), None, None, _stream(stream)))
        ring, counters = np.zeros(s.capacity, np.float32), np.zeros(self.max_levels + 2, np.uint32)
        check(lib.mi_qcounter_bank_get_state(self.handle, channel, byref(s), ring.ctypes.data_as(c_void_p), counters.ctypes.data_as(c_void_p),
                                             _stream(stream)))
        return {"head": s.head, "count": s.count, "capacity": s.capacity, "ring": ring, "counters": counters}

    def set_state(self, channel, head, count, ring=None, counters=None, stream=None):
        from .capi import QuantizedCounterState
        s = QuantizedCounterState(head, count, 0)
        r = None if ring is None else np.ascontiguousarray(ring, np.float32)
        c = None if counters is None else np.ascontiguousarray(counters, np.uint32)
        check(lib.mi_qcounter_bank_set_state(self.handle, channel, byref(s), None if r is None else r.ctypes.data_as(c_void_p),
                                             None if c is None else c.ctypes.data_as(c_void_p), _stream(stream)))

    def close(self):
        if self.handle:
            lib.mi_qcounter_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SurgeProtectorBank:
    """`channels` x lsp::dspu::SurgeProtector (mi_surge_bank_*): a fade-in when the level row appears, a fade-out when it stops."""
    ALL = 0xFFFFFFFF

    def __init__(self, channels):
        h = c_void_p()
        check(lib.mi_surge_bank_create(byref(h), channels))
        self.handle, self.channels = h, channels

    def set_transition_time(self, channel, samples):
        check(lib.mi_surge_bank_set_transition_time(self.handle, channel, samples))

    def set_shutdown_time(self, channel, samples):
        check(lib.mi_surge_bank_set_shutdown_time(self.handle, channel, samples))

    def set_on_threshold(self, channel, threshold):
        check(lib.mi_surge_bank_set_on_threshold(self.handle, channel, float(threshold)))

    def set_off_threshold(self, channel, threshold):
        check(lib.mi_surge_bank_set_off_threshold(self.handle, channel, float(threshold)))

    def set_threshold(self, channel, on, off):
        check(lib.mi_surge_bank_set_threshold(self.handle, channel, float(on), float(off)))

    def configure(self, channel, transition, shutdown, on, off):
        """Every setter of one channel (times in samples)."""
        self.set_transition_time(channel, transition)
        self.set_shutdown_time(channel, shutdown)
        self.set_threshold(channel, on, off)

    def reset(self, channel=ALL):
        check(lib.mi_surge_bank_reset(self.handle, channel))

    def get_params(self, channel):
        from .capi import SurgeParams
        p = SurgeParams()
        check(lib.mi_surge_bank_get_params(self.handle, channel, byref(p)))
        return {"transition_max": p.transition_max, "shutdown_max": p.shutdown_max, "on_threshold": np.float32(p.on_threshold),
                "off_threshold": np.float32(p.off_threshold)}

    def get_state(self, channel, stream=None):
        from .capi import SurgeState
        s = SurgeState()
        check(lib.mi_surge_bank_get_state(self.handle, channel, byref(s), _stream(stream)))
        return {"gain": np.float32(s.gain), "transition_time": s.transition_time, "shutdown_time": s.shutdown_time, "on": s.on}

    def set_state(self, channel, gain, transition_time, shutdown_time, on, stream=None):
        from .capi import SurgeState
        s = SurgeState(float(gain), transition_time, shutdown_time, int(on))
        check(lib.mi_surge_bank_set_state(self.handle, channel, byref(s), _stream(stream)))

    def process(self, out, inp, count, out_stride=None, in_stride=None, stream=None):
        """process(out, in, count): the gain into out; out None: the state only; out may be inp."""
        check(lib.mi_surge_bank_process(self.handle, _opt(out), _opt(inp), count, count if out_stride is None else out_stride,
                                        count if in_stride is None else in_stride, _stream(stream)))

    def process_mul(self, out, inp, count, out_stride=None, in_stride=None, stream=None):
        """process_mul(out, in, count): out *= gain; out may be inp."""
        check(lib.mi_surge_bank_process_mul(self.handle, _opt(out), _opt(inp), count, count if out_stride is None else out_stride,
                                            count if in_stride is None else in_stride, _stream(stream)))

    def close(self):
        if self.handle:
            lib.mi_surge_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DepopperBank:
    """`channels` x lsp::dspu::Depopper (mi_depopper_bank_*): the RMS envelope of a row and a gain that fades in when the signal
    appears and -- ahead of time, by the look-ahead -- out before it vanishes."""
    MODES = {"linear": 0, "cubic": 1, "sine": 2, "gaussian": 3, "parabolic": 4}

    def __init__(self, channels):
        h = c_void_p()
        check(lib.mi_depopper_bank_create(byref(h), channels))
        self.handle, self.channels = h, channels

    def init(self, channel, sample_rate, max_fade, max_rms):
        check(lib.mi_depopper_bank_init(self.handle, channel, sample_rate, float(max_fade), float(max_rms)))

    def _set_mode(self, fn, channel, mode):
        old = c_uint32()
        check(fn(self.handle, channel, self.MODES.get(mode, mode), byref(old)))
        return old.value

    def _set_float(self, fn, channel, value):
        old = c_float()
        check(fn(self.handle, channel, float(value), byref(old)))
        return np.float32(old.value)

    def set_fade_in_mode(self, channel, mode):
        return self._set_mode(lib.mi_depopper_bank_set_fade_in_mode, channel, mode)

    def set_fade_out_mode(self, channel, mode):
        return self._set_mode(lib.mi_depopper_bank_set_fade_out_mode, channel, mode)

    def set_fade_in_time(self, channel, time):
        return self._set_float(lib.mi_depopper_bank_set_fade_in_time, channel, time)

    def set_fade_out_time(self, channel, time):
        return self._set_float(lib.mi_depopper_bank_set_fade_out_time, channel, time)

    def set_fade_in_threshold(self, channel, threshold):
        return self._set_float(lib.mi_depopper_bank_set_fade_in_threshold, channel, threshold)

    def set_fade_out_threshold(self, channel, threshold):
        return self._set_float(lib.mi_depopper_bank_set_fade_out_threshold, channel, threshold)

    def set_fade_in_delay(self, channel, delay):
        return self._set_float(lib.mi_depopper_bank_set_fade_in_delay, channel, delay)

    def set_fade_out_delay(self, channel, delay):
        return self._set_float(lib.mi_depopper_bank_set_fade_out_delay, channel, delay)

    def set_rms_length(self, channel, length):
        return self._set_float(lib.mi_depopper_bank_set_rms_length, channel, length)

    def update_settings(self, stream=None):
        check(lib.mi_depopper_bank_update_settings(self.handle, _stream(stream)))

    @staticmethod
    def _fade(f):
        return {"mode": f.mode, "threshold": np.float32(f.threshold), "time": np.float32(f.time), "delay": np.float32(f.delay),
                "samples": f.samples, "delay_samples": f.delay_samples, "poly": np.array(list(f.poly), np.float32)}

    def get_params(self, channel):
        """The reference's designed fields as the last update_settings() left them."""
        from .capi import DepopperParams
        p = DepopperParams()
        check(lib.mi_depopper_bank_get_params(self.handle, channel, byref(p)))
        return {"fade_in": self._fade(p.fade_in), "fade_out": self._fade(p.fade_out), "sample_rate": p.sample_rate,
                "look_max": np.float32(p.look_max), "rms_max": np.float32(p.rms_max), "rms_length": np.float32(p.rms_length),
                "rms_norm": np.float32(p.rms_norm), "look_min_off": p.look_min_off, "look_max_off": p.look_max_off,
                "look_count": p.look_count, "rms_min_off": p.rms_min_off, "rms_max_off": p.rms_max_off, "rms_len": p.rms_len,
                "reconfigure": p.reconfigure}

    def get_fade_table(self, channel, fade_out):
        """crossfade(sFadeOut if fade_out else sFadeIn, x) for x = 0 .. nSamples - 1, as the device reads it."""
        n = ctypes.c_size_t()
        check(lib.mi_depopper_bank_get_fade_table(self.handle, channel, int(bool(fade_out)), None, 0, byref(n)))
        t = np.zeros(n.value, np.float32)
        check(lib.mi_depopper_bank_get_fade_table(self.handle, channel, int(bool(fade_out)), c_void_p(t.ctypes.data), t.size, byref(n)))
        return t

    def latency(self, channel):
        n = ctypes.c_int64()
        check(lib.mi_depopper_bank_latency(self.handle, channel, byref(n)))
        return n.value

    def get_state(self, channel, buffers=False, stream=None):
        """fRms, nState, nCounter, nDelay, nRmsOff, nLookOff; with buffers also the last nRmsMin squares and nLookMin gains."""
        from .capi import DepopperState
        s = DepopperState()
        rms = gain = None
        if buffers:
            p = self.get_params(channel)
            rms, gain = np.zeros(p["rms_min_off"], np.float32), np.zeros(p["look_min_off"], np.float32)
        check(lib.mi_depopper_bank_get_state(self.handle, channel, byref(s), c_void_p(rms.ctypes.data) if buffers else None,
                                             c_void_p(gain.ctypes.data) if buffers else None, _stream(stream)))
        out = {"rms": np.float32(s.rms), "state": s.state, "counter": s.counter, "delay": s.delay, "rms_off": s.rms_off,
               "look_off": s.look_off}
        if buffers:
            out["rms_buf"], out["gain_buf"] = rms, gain
        return out

    def set_state(self, channel, rms, state, counter, delay, rms_off, look_off, rms_buf=None, gain_buf=None, stream=None):
        from .capi import DepopperState
        s = DepopperState(float(rms), state, counter, delay, rms_off, look_off)
        rb = None if rms_buf is None else np.ascontiguousarray(rms_buf, np.float32)
        gb = None if gain_buf is None else np.ascontiguousarray(gain_buf, np.float32)
        check(lib.mi_depopper_bank_set_state(self.handle, channel, byref(s), None if rb is None else c_void_p(rb.ctypes.data),
                                             None if gb is None else c_void_p(gb.ctypes.data), _stream(stream)))

    def process(self, env, gain, src, count, env_stride=None, gain_stride=None, src_stride=None, stream=None):
        """process(env, gain, src, count): env may be None; env or gain may be src."""
        check(lib.mi_depopper_bank_process(self.handle, _opt(env), _opt(gain), _opt(src), count,
                                           count if env_stride is None else env_stride, count if gain_stride is None else gain_stride,
                                           count if src_stride is None else src_stride, _stream(stream)))

    def close(self):
        if self.handle:
            lib.mi_depopper_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _word_and_floats(struct, word, a, b):
    """A state struct of one uint32 and two float32 with the floats' bits as given (a NaN keeps its payload)."""
    return struct.from_buffer_copy(np.uint32(word).tobytes() + np.float32(a).tobytes() + np.float32(b).tobytes())


class BypassBank:
    """`channels` x lsp::dspu::Bypass (mi_bypass_bank_*): a click-free switch between a dry and a wet row, nState, fDelta and
    fGain on the device."""
    ALL = 0xFFFFFFFF
    S_ON, S_ACTIVE, S_OFF = 0, 1, 2

    def __init__(self, channels):
        h = c_void_p()
        check(lib.mi_bypass_bank_create(byref(h), channels))
        self.handle, self.channels = h, channels

    def init(self, channel, sample_rate, time=0.005):
        check(lib.mi_bypass_bank_init(self.handle, channel, int(sample_rate), float(time)))

    def set_bypass(self, channel, bypass):
        """set_bypass(bypass): whether the channel changed direction; for ALL, how many did."""
        n = c_int()
        check(lib.mi_bypass_bank_set_bypass(self.handle, channel, 1 if bypass else 0, byref(n)))
        return n.value if channel == self.ALL else bool(n.value)

    def bypassing(self, channel, stream=None):
        v = c_int()
        check(lib.mi_bypass_bank_bypassing(self.handle, channel, byref(v), _stream(stream)))
        return bool(v.value)

    def get_state(self, channel, stream=None):
        from .capi import BypassState
        s = BypassState()
        check(lib.mi_bypass_bank_get_state(self.handle, channel, byref(s), _stream(stream)))
        return {"state": s.state, "delta": np.frombuffer(bytes(s), np.float32)[1], "gain": np.frombuffer(bytes(s), np.float32)[2]}

    def set_state(self, channel, state, delta, gain, stream=None):
        from .capi import BypassState
        s = _word_and_floats(BypassState, state, delta, gain)
        check(lib.mi_bypass_bank_set_state(self.handle, channel, byref(s), _stream(stream)))

    @staticmethod
    def _rows(count, dst_stride, dry_stride, wet_stride):
        """count and the three strides of a process call, each stride `count` where it is not given"""
        return (count, count if dst_stride is None else dst_stride, count if dry_stride is None else dry_stride,
                count if wet_stride is None else wet_stride)

    def process(self, dst, dry, wet, count, dst_stride=None, dry_stride=None, wet_stride=None, stream=None):
        """process(dst, dry, wet, count); dry may be None; dst may be dry or wet."""
        check(lib.mi_bypass_bank_process(self.handle, _opt(dst), _opt(dry), _opt(wet),
                                         *self._rows(count, dst_stride, dry_stride, wet_stride), _stream(stream)))

    def process_wet(self, dst, dry, wet, wet_gain, count, dst_stride=None, dry_stride=None, wet_stride=None, stream=None):
        check(lib.mi_bypass_bank_process_wet(self.handle, _opt(dst), _opt(dry), _opt(wet), float(wet_gain),
                                             *self._rows(count, dst_stride, dry_stride, wet_stride), _stream(stream)))

    def process_drywet(self, dst, dry, wet, dry_gain, wet_gain, count, dst_stride=None, dry_stride=None, wet_stride=None, stream=None):
        check(lib.mi_bypass_bank_process_drywet(self.handle, _opt(dst), _opt(dry), _opt(wet), float(dry_gain), float(wet_gain),
                                                *self._rows(count, dst_stride, dry_stride, wet_stride), _stream(stream)))

    def close(self):
        if self.handle:
            lib.mi_bypass_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CrossfadeBank:
    """`channels` x lsp::dspu::Crossfade (mi_crossfade_bank_*): after toggle() the output goes from fade_out to fade_in."""
    ALL = 0xFFFFFFFF

    def __init__(self, channels):
        h = c_void_p()
        check(lib.mi_crossfade_bank_create(byref(h), channels))
        self.handle, self.channels = h, channels

    def init(self, channel, sample_rate, time=0.005):
        check(lib.mi_crossfade_bank_init(self.handle, channel, int(sample_rate), float(time)))

    def toggle(self, channel):
        """toggle(): whether a fade started; for ALL, on how many channels."""
        n = c_int()
        check(lib.mi_crossfade_bank_toggle(self.handle, channel, byref(n)))
        return n.value if channel == self.ALL else bool(n.value)

    def reset(self, channel=ALL):
        check(lib.mi_crossfade_bank_reset(self.handle, channel))

    def remaining(self, channel):
        from ctypes import c_size_t
        v = c_size_t()
        check(lib.mi_crossfade_bank_remaining(self.handle, channel, byref(v)))
        return v.value

    def get_state(self, channel, stream=None):
        from .capi import CrossfadeState
        s = CrossfadeState()
        check(lib.mi_crossfade_bank_get_state(self.handle, channel, byref(s), _stream(stream)))
        return {"counter": s.counter, "delta": np.frombuffer(bytes(s), np.float32)[1], "gain": np.frombuffer(bytes(s), np.float32)[2]}

    def set_state(self, channel, counter, delta, gain, stream=None):
        from .capi import CrossfadeState
        s = _word_and_floats(CrossfadeState, counter, delta, gain)
        check(lib.mi_crossfade_bank_set_state(self.handle, channel, byref(s), _stream(stream)))

    def process(self, dst, fade_out, fade_in, count, dst_stride=None, out_stride=None, in_stride=None, stream=None):
        """process(dst, fade_out, fade_in, count); either input may be None, or both; dst may be either input."""
        check(lib.mi_crossfade_bank_process(self.handle, _opt(dst), _opt(fade_out), _opt(fade_in), count,
                                            count if dst_stride is None else dst_stride, count if out_stride is None else out_stride,
                                            count if in_stride is None else in_stride, _stream(stream)))

    def close(self):
        if self.handle:
            lib.mi_crossfade_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LoudnessBank:
    """`meters` x lsp::dspu::LoudnessMeter(channels) sharing one configuration (mi_loudness_bank_*)."""
    WEIGHT_NONE, WEIGHT_A, WEIGHT_B, WEIGHT_C, WEIGHT_D, WEIGHT_K = range(6)

    def __init__(self, meters, channels, max_period_ms=400.0):
        h = c_void_p()
        check(lib.mi_loudness_bank_create(byref(h), meters, channels, float(max_period_ms)))
        self.handle, self.meters, self.channels = h, meters, channels

    def set_sample_rate(self, sr, stream=None):
        check(lib.mi_loudness_bank_set_sample_rate(self.handle, sr, _stream(stream)))

    def set_period(self, ms):
        check(lib.mi_loudness_bank_set_period(self.handle, float(ms)))

    def set_weighting(self, w):
        check(lib.mi_loudness_bank_set_weighting(self.handle, int(w)))

    def set_designation(self, channel, designation):
        check(lib.mi_loudness_bank_set_designation(self.handle, channel, int(designation)))

    def set_link(self, channel, link):
        check(lib.mi_loudness_bank_set_link(self.handle, channel, float(link)))

    def set_active(self, channel, active=True, stream=None):
        check(lib.mi_loudness_bank_set_active(self.handle, channel, 1 if active else 0, _stream(stream)))

    def set_bound(self, channel, bound=True):
        check(lib.mi_loudness_bank_set_bound(self.handle, channel, 1 if bound else 0))

    def clear(self, stream=None):
        check(lib.mi_loudness_bank_clear(self.handle, _stream(stream)))

    def latency(self):
        v = c_uint32()
        check(lib.mi_loudness_bank_latency(self.handle, byref(v)))
        return v.value

    def process(self, out, ch_out, inp, count, out_stride=None, in_stride=None, gain=None, stream=None):
        """gain=None: process(out, count), which also records loudness(); a number: process(out, count, gain)."""
        args = (self.handle, _ptr(out) if out is not None else None, _ptr(ch_out) if ch_out is not None else None, _ptr(inp),
                count, count if out_stride is None else out_stride, count if in_stride is None else in_stride)
        if gain is None:
            check(lib.mi_loudness_bank_process(*args, _stream(stream)))
        else:
            check(lib.mi_loudness_bank_process_gain(*args, float(gain), _stream(stream)))

    def set_exact(self, on=True):
        check(lib.mi_loudness_bank_set_exact(self.handle, 1 if on else 0))

    def loudness(self, stream=None):
        v = (c_float * self.meters)()
        check(lib.mi_loudness_bank_loudness(self.handle, v, _stream(stream)))
        return np.array(list(v), np.float32)

    def close(self):
        if self.handle:
            lib.mi_loudness_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ILUFSBank:
    """`meters` x lsp::dspu::ILUFSMeter(channels) sharing one configuration (mi_ilufs_bank_*)."""
    DBFS_TO_LUFS_SHIFT_GAIN = 0.923527857225

    def __init__(self, meters, channels, max_int_time=60.0, block_period_ms=400.0):
        h = c_void_p()
        check(lib.mi_ilufs_bank_create(byref(h), meters, channels, float(max_int_time), float(block_period_ms)))
        self.handle, self.meters, self.channels = h, meters, channels

    def set_sample_rate(self, sr, stream=None):
        check(lib.mi_ilufs_bank_set_sample_rate(self.handle, sr, _stream(stream)))

    def set_integration_period(self, seconds, stream=None):
        check(lib.mi_ilufs_bank_set_integration_period(self.handle, float(seconds), _stream(stream)))

    def set_weighting(self, w):
        check(lib.mi_ilufs_bank_set_weighting(self.handle, int(w)))

    def set_designation(self, channel, designation):
        check(lib.mi_ilufs_bank_set_designation(self.handle, channel, int(designation)))

    def set_active(self, channel, active=True):
        check(lib.mi_ilufs_bank_set_active(self.handle, channel, 1 if active else 0))

    def clear(self, stream=None):
        check(lib.mi_ilufs_bank_clear(self.handle, _stream(stream)))

    def process(self, out, inp, count, out_stride=None, in_stride=None, gain=DBFS_TO_LUFS_SHIFT_GAIN, stream=None):
        check(lib.mi_ilufs_bank_process(self.handle, _ptr(out) if out is not None else None, _ptr(inp), count,
                                        count if out_stride is None else out_stride,
                                        count if in_stride is None else in_stride, float(gain), _stream(stream)))

    def set_exact(self, on=True):
        check(lib.mi_ilufs_bank_set_exact(self.handle, 1 if on else 0))

    def loudness(self, stream=None):
        v = (c_float * self.meters)()
        check(lib.mi_ilufs_bank_loudness(self.handle, v, _stream(stream)))
        return np.array(list(v), np.float32)

    def history(self, stream=None):
        """(hist [meters][size], head [meters], count [meters]) as the meters hold them."""
        size = c_uint32()
        check(lib.mi_ilufs_bank_history(self.handle, None, byref(size), None, None, _stream(stream)))
        hist = np.zeros((self.meters, size.value), np.float32)
        head = (c_uint32 * self.meters)()
        count = (c_uint32 * self.meters)()
        check(lib.mi_ilufs_bank_history(self.handle, hist.ctypes.data_as(c_void_p) if size.value else None, byref(size), head, count,
                                        _stream(stream)))
        return hist, np.array(head[:], np.int64), np.array(count[:], np.int64)

    def close(self):
        if self.handle:
            lib.mi_ilufs_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SplitterBank:
    """lsp::dspu::SpectralSplitter for `channels` channels sharing the settings (mi_splitter_bank_*)."""

    def __init__(self, channels, max_rank, handlers):
        h = c_void_p()
        check(lib.mi_splitter_bank_create(byref(h), channels, max_rank, handlers))
        self.handle, self.channels, self.handlers = h, channels, handlers
        self._cbs = {}

    def set_rank(self, rank):
        check(lib.mi_splitter_bank_set_rank(self.handle, rank))

    def set_chunk_rank(self, rank):
        check(lib.mi_splitter_bank_set_chunk_rank(self.handle, rank))

    def set_phase(self, phase):
        check(lib.mi_splitter_bank_set_phase(self.handle, float(phase)))

    def _get(self):
        v = [c_uint32() for _ in range(4)]
        check(lib.mi_splitter_bank_get(self.handle, *[byref(x) for x in v]))
        return [x.value for x in v]

    def rank(self):
        return self._get()[0]

    def chunk_rank(self):
        return self._get()[1]

    def latency(self):
        return self._get()[2]

    def remaining(self):
        return self._get()[3]

    def bind_copy(self, handler, stream=None):
        check(lib.mi_splitter_bank_bind_copy(self.handle, handler, _stream(stream)))

    def bind_mask(self, handler, mask, stream=None):
        """mask: 2^rank gains (shared) or [channels][2^rank], host array."""
        from ctypes import POINTER as _P
        m = np.ascontiguousarray(mask, dtype=np.float32)
        stride = 0 if m.ndim == 1 else m.shape[1]
        check(lib.mi_splitter_bank_bind_mask(self.handle, handler, m.ctypes.data_as(_P(c_float)), stride, _stream(stream)))

    def bind_callback(self, handler, pyfunc, stream=None):
        """pyfunc(out_ptr, in_ptr, rank, channels, stream): device addresses of [channels][2 * 2^rank] floats."""
        from ctypes import cast
        from .capi import SPLITTER_FUNC
        cb = SPLITTER_FUNC(lambda obj, subj, out, inp, rank, ch, st: pyfunc(out, inp, rank, ch, st))
        self._cbs[handler] = cb
        check(lib.mi_splitter_bank_bind_callback(self.handle, handler, cast(cb, c_void_p), None, None, _stream(stream)))

    def unbind(self, handler):
        check(lib.mi_splitter_bank_unbind(self.handle, handler))
        self._cbs.pop(handler, None)

    def clear(self, stream=None):
        check(lib.mi_splitter_bank_clear(self.handle, _stream(stream)))

    def process(self, outs, inp, count, out_stride=None, in_stride=None, stream=None):
        """outs: list of `handlers` device buffers or None (handler without a sink); inp None = silence."""
        arr = (c_void_p * self.handlers)(*[(_ptr(b) if b is not None else None) for b in outs])
        check(lib.mi_splitter_bank_process(self.handle, arr, _ptr(inp) if inp is not None else None, count,
                                           count if out_stride is None else out_stride,
                                           count if in_stride is None else in_stride, _stream(stream)))

    def process_blocks(self, outs, inps, count, out_stride=None, in_stride=None, stream=None):
        """len(inps) consecutive process() calls in one C call; outs[k]: block k's list of `handlers` buffers (or None)."""
        n = len(inps)
        assert n == len(outs)
        flat = [(_ptr(b) if b is not None else None) for o in outs for b in o]
        assert len(flat) == n * self.handlers
        po = (c_void_p * len(flat))(*flat)
        pi = (c_void_p * n)(*[_ptr(b) for b in inps])
        check(lib.mi_splitter_bank_process_blocks(self.handle, po, pi, n, count,
                                                  count if out_stride is None else out_stride,
                                                  count if in_stride is None else in_stride, _stream(stream)))

    def close(self):
        if self.handle:
            lib.mi_splitter_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def crossover_fft_mask(hpf, lpf, flatten, gain, sample_rate, rank):
    """FFTCrossover::update_band (FFTCrossover.cpp:459-486): hpf / lpf = (freq, slope) or None."""
    from ctypes import POINTER as _P
    n = 1 << rank
    m = np.empty(n, np.float32)
    p = m.ctypes.data_as(_P(c_float))
    if hpf is not None:
        lib.mi_crossover_hipass_fft_set(p, hpf[0], hpf[1], float(sample_rate), rank)
        if lpf is not None:
            lib.mi_crossover_lopass_fft_apply(p, lpf[0], lpf[1], float(sample_rate), rank)
    elif lpf is not None:
        lib.mi_crossover_lopass_fft_set(p, lpf[0], lpf[1], float(sample_rate), rank)
    else:
        m[:] = np.float32(flatten) * np.float32(gain)
        return m
    return (np.clip(m, np.float32(0.0), np.float32(flatten)) * np.float32(gain)).astype(np.float32)


class CrossoverBank:
    """lsp::dspu::Crossover for `channels` channels sharing the split settings (mi_crossover_bank_*)."""
    MODE_BT, MODE_MT = 0, 1

    def __init__(self, channels, bands):
        h = c_void_p()
        check(lib.mi_crossover_bank_create(byref(h), channels, bands))
        self.handle, self.channels, self.bands = h, channels, bands

    def set_sample_rate(self, sr):
        check(lib.mi_crossover_bank_set_sample_rate(self.handle, sr))

    def set_slope(self, split, slope):
        check(lib.mi_crossover_bank_set_slope(self.handle, split, slope))

    def set_frequency(self, split, freq):
        check(lib.mi_crossover_bank_set_frequency(self.handle, split, float(freq)))

    def set_mode(self, split, mode):
        check(lib.mi_crossover_bank_set_mode(self.handle, split, mode))

    def set_gain(self, band, gain):
        check(lib.mi_crossover_bank_set_gain(self.handle, band, float(gain)))

    def get_split(self, split):
        sl, fr, mo = c_uint32(), c_float(), c_int()
        check(lib.mi_crossover_bank_get_split(self.handle, split, byref(sl), byref(fr), byref(mo)))
        return {"slope": sl.value, "freq": fr.value, "mode": mo.value}

    def get_band(self, band, stream=None):
        g, s0, s1, act = c_float(), c_float(), c_float(), c_int()
        check(lib.mi_crossover_bank_get_band(self.handle, band, byref(g), byref(s0), byref(s1), byref(act), _stream(stream)))
        return {"gain": g.value, "start": s0.value, "end": s1.value, "active": bool(act.value)}

    def process(self, band_out, inp, samples, out_stride=None, in_stride=None, stream=None):
        """band_out: list of `bands` device buffers or None (band without a handler)."""
        arr = (c_void_p * self.bands)(*[(_ptr(b) if b is not None else None) for b in band_out])
        check(lib.mi_crossover_bank_process(self.handle, arr, _ptr(inp), samples,
                                            samples if out_stride is None else out_stride,
                                            samples if in_stride is None else in_stride, _stream(stream)))

    def process_blocks(self, band_outs, inps, samples, out_stride=None, in_stride=None, stream=None):
        """len(inps) consecutive process() calls in one C call; band_outs[i]: block i's list of `bands` buffers (or None)."""
        n = len(inps)
        assert n == len(band_outs)
        flat = [(_ptr(b) if b is not None else None) for outs in band_outs for b in outs]
        assert len(flat) == n * self.bands
        po = (c_void_p * len(flat))(*flat)
        pi = (c_void_p * n)(*[_ptr(b) for b in inps])
        check(lib.mi_crossover_bank_process_blocks(self.handle, po, pi, n, samples,
                                                   samples if out_stride is None else out_stride,
                                                   samples if in_stride is None else in_stride, _stream(stream)))

    def freq_chart(self, band, freqs, stream=None):
        import numpy as np
        f = np.ascontiguousarray(freqs, dtype=np.float32)
        c = np.empty(2 * f.size, np.float32)
        from ctypes import POINTER as _P
        check(lib.mi_crossover_bank_freq_chart(self.handle, band, c.ctypes.data_as(_P(c_float)),
                                               f.ctypes.data_as(_P(c_float)), f.size, _stream(stream)))
        return c[0::2] + 1j * c[1::2]

    def close(self):
        if self.handle:
            lib.mi_crossover_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EqualizerBank:
    """`channels` x lsp::dspu::Equalizer on the device."""
    BYPASS, IIR, FIR, FFT, SPM = range(5)

    def __init__(self, channels, filters, fir_rank):
        h = c_void_p()
        check(lib.mi_equalizer_bank_create(byref(h), channels, filters, fir_rank))
        self.handle, self.channels = h, channels

    def set_params(self, filter_id, ftype, slope=1, freq=1000.0, freq2=1000.0, gain=1.0, quality=0.0, channel=None):
        fp = FilterParams(int(ftype), int(slope), float(freq), float(freq2), float(gain), float(quality))
        check(lib.mi_equalizer_bank_set_params(self.handle, 0xFFFFFFFF if channel is None else channel, filter_id, byref(fp)))

    def set_mode(self, mode):
        check(lib.mi_equalizer_bank_set_mode(self.handle, mode))

    def set_sample_rate(self, sr):
        check(lib.mi_equalizer_bank_set_sample_rate(self.handle, sr))

    def get_latency(self, stream=None):
        v = c_uint32()
        check(lib.mi_equalizer_bank_get_latency(self.handle, byref(v), _stream(stream)))
        return v.value

    def set_smooth(self, smooth):
        """Equalizer::set_smooth: FIR/FFT retunes cross-fade over the block that completes next."""
        check(lib.mi_equalizer_bank_set_smooth(self.handle, 1 if smooth else 0))

    def reset(self, stream=None):
        check(lib.mi_equalizer_bank_reset(self.handle, _stream(stream)))

    def process(self, out, inp, samples, out_stride=None, in_stride=None, stream=None):
        check(lib.mi_equalizer_bank_process(self.handle, _ptr(out), _ptr(inp), samples,
                                            samples if out_stride is None else out_stride,
                                            samples if in_stride is None else in_stride, _stream(stream)))

    def process_blocks(self, outs, inps, samples, out_stride=None, in_stride=None, stream=None):
        """len(outs) consecutive process() calls issued by one C call (mi_equalizer_bank_process_blocks)."""
        n = len(outs)
        assert n == len(inps)
        po = (c_void_p * n)(*[_ptr(b) for b in outs])
        pi = (c_void_p * n)(*[_ptr(b) for b in inps])
        check(lib.mi_equalizer_bank_process_blocks(self.handle, po, pi, n, samples,
                                                   samples if out_stride is None else out_stride,
                                                   samples if in_stride is None else in_stride, _stream(stream)))

    def close(self):
        if self.handle:
            lib.mi_equalizer_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
