"""ctypes binding of libdpemu.so (include/dpemu.h).  No fallback: if the HIP
library is missing or a GPU call fails, this raises."""

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, 'libdpemu.so')

_vp, _u32, _u64, _int = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int

# every entry point declared in include/dpemu.h: name -> (argtypes, restype)
SIGNATURES = {
    'dpemu_abi_version': ([], _int),
    'dpemu_struct_sizes': ([_vp], _int),
    'dpemu_create': ([_int, C.POINTER(_vp)], _int),
    'dpemu_destroy': ([_vp], _int),
    'dpemu_last_error': ([_vp], C.c_char_p),
    'dpemu_load_programs': ([_vp, _vp, _u64, _vp, _vp, _u32, _vp, _u32, _u32], _int),
    'dpemu_load_readout_freqs': ([_vp, _vp, _u64, _vp, _vp, _vp, _vp], _int),
    'dpemu_run': ([_vp, _vp, _u64, _u64, _vp, _vp], _int),
    'dpemu_run_states': ([_vp, _vp, _u64, _u64, _vp, _vp, _vp], _int),   # dpemu_run + states before the stream
    'dpemu_run_host': ([_vp, _vp, _u64, _u64, _vp], _int),
    'dpemu_dds': ([_vp] * 8, _int),
    'dpemu_dds_sin_lut': ([_vp], _int),
    'dpemu_demod_iq': ([_vp] * 10, _int),
    'dpemu_feedline_adc': ([_vp] * 9, _int),
    'dpemu_feedline_adc_res': ([_vp] * 10, _int),
    'dpemu_demod_feedline': ([_vp] * 11, _int),
    'dpemu_feedline_traces': ([_vp] * 11, _int),
    'dpemu_iq_stats': ([_vp] * 8, _int),
    'dpemu_qsim': ([_vp] * 8, _int),
    'dpemu_qsim_phase_lut': ([_vp], _int),
    'dpemu_qsim_meas': ([_vp] * 9, _int),
    'dpemu_qsim_decay': ([_vp] * 11, _int),           # dec after qs; states and counts before the stream
    'dpemu_set_kernel_timing': ([_vp, _int], _int),
    'dpemu_kernel_times': ([_vp, _vp, _int, _vp], _int),
    'dpemu_last_kernel': ([_vp], C.c_char_p),
}
# a *_st entry point is its base with the states pointer before the stream
ST_BASES = ('dpemu_feedline_adc', 'dpemu_feedline_adc_res', 'dpemu_feedline_traces', 'dpemu_iq_stats')
SIGNATURES.update({b + '_st': (SIGNATURES[b][0][:-1] + [_vp, _vp], SIGNATURES[b][1]) for b in ST_BASES})
EXPORTS = tuple(SIGNATURES)

_libs = {}


class DpemuError(RuntimeError):
    pass


def load_library(path=LIB_PATH):
    """the ctypes handle of libdpemu.so (another build's path for A/B runs)"""
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise DpemuError('libdpemu.so not built ({}); run __graft_entry__.build() '
                         '(hipcc --offload-arch=gfx950)'.format(path))
    # One HIP runtime per process.  PyTorch-ROCm ships its own
    # libamdhip64.so (soname libamdhip64.so.7) and libhsa-runtime64; loaded
    # first, it satisfies libdpemu.so's libamdhip64.so.7 dependency, so both
    # share one runtime and device pointers / streams pass freely.  Loaded
    # after ours, torch would bring up a second runtime that finds no GPU.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(path)
    # an older build lacks later entry points: name them instead of letting
    # ctypes raise a bare AttributeError on the first argtypes assignment
    missing = [s for s in EXPORTS if not hasattr(L, s)]
    if missing:
        raise DpemuError('{} lacks {} (a build older than this binding); rebuild it with '
                         '__graft_entry__.build()'.format(path, ', '.join(missing)))
    for name, (argtypes, restype) in SIGNATURES.items():
        f = getattr(L, name)
        f.argtypes, f.restype = argtypes, restype
    from . import _abi
    if L.dpemu_abi_version() != _abi.ABI_VERSION:
        raise DpemuError('ABI version mismatch: library {} vs host {}'.format(
            L.dpemu_abi_version(), _abi.ABI_VERSION))
    # the struct layouts too: two builds of one ABI version from different
    # header states must not share a process with a mismatched ctypes mirror
    sizes = (C.c_uint64 * 3)()
    L.dpemu_struct_sizes(sizes)
    mine = (C.sizeof(_abi.Config), C.sizeof(_abi.Outputs), C.sizeof(_abi.DDSChannels))
    if tuple(sizes) != mine:
        raise DpemuError('struct layout mismatch: library {} vs host {} ({})'.format(tuple(sizes), mine, path))
    _libs[path] = L
    return L


def check(ctx_handle, rc, what, L=None):
    if rc != 0:
        L = L or load_library()
        msg = L.dpemu_last_error(ctx_handle)
        raise DpemuError('{} failed ({}): {}'.format(what, rc, msg.decode() if msg else ''))
