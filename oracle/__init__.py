"""
ORACLE package -- test infrastructure only.

CPU restatement of the reference's hot-path algorithms (C in *.c, the filter
designer in filter_design.py).  Only tests/, __graft_entry__.smoke() and the
cpu_baseline leg of bench.py may import this package; the product
(lsp-dsp-units_amd/) never does.

The reference as a whole cannot be built in this environment: its arithmetic core
(lsp-dsp-lib 1.0.36) and lsp-common-lib/lsp-runtime-lib/lsp-lltl-lib/lsp-test-fw
are un-vendored (modules.mk:23-51, fetched by `make fetch`) and absent.  Each
restated function cites the reference file:line it follows and is pinned against
the reference's own unit-test expectations (tests/test_oracle_*.py).

Four classes are built from the reference's own text, because their logic lives
in their .cpp files and not in the absent libraries: Compressor, Expander, Gate
and DynamicProcessor (Makefile -> _ref/dyn_ref, with the stand-in headers of
ref_shim/ and the driver dyn_driver.cpp; _ref/ is never committed).  That pins
their followers, hold, hysteresis, update_settings and scalar gain formulas
(tests/golden/dynamics_ref_vectors.npz, tests/test_dynamics_reference_*.py).
Three more likewise, Limiter, AutoGain and SimpleAutoGain (Makefile -> _ref/gain_ref and its
sanitizer twin _ref/gain_ref_san, driver gain_driver.cpp; tests/golden/
limiter_ref_vectors.npz and autogain_ref_vectors.npz, tests/test_gain_reference_*.py).
Filter, FilterBank and DynamicFilters likewise (Makefile -> _ref/filter_ref, _ref/dynfilter_ref and
their sanitizer twins, drivers filter_driver.cpp and dynfilter_driver.cpp, stand-ins in
ref_overlay/filters/; tests/golden/filter_ref_*.npz and dynfilter_ref_*.npz,
tests/test_filter_reference_*.py and tests/test_dynfilter_reference_*.py): the designer,
Filter::limit, the bank's packing and clear / keep rules, the dynamic cascade builders.
LoudnessMeter and ILUFSMeter likewise, with the reference's own Filter, FilterBank and
designation table (Makefile -> _ref/loudness_ref and _ref/loudness_ref_san, driver
loudness_driver.cpp, stand-ins in ref_overlay/meters/; tests/golden/loudness_ref_vectors.npz
and ilufs_ref_vectors.npz, tests/test_loudness_reference_*.py): the ring and its refresh
schedule, the two process() forms, linking, binding and nOffset, the gating blocks, the
lost F_BLK_FULL, the history and its halving.  Not pinned there: the summation order of
dsp::h_sum / h_sqr_sum, the result type of the mixed lsp_min, DEFAULT_ALIGN (0x40: the
length of the ILUFSMeter's history) -- and LoudnessMeter::clear(), which the reference
leaves ill-defined (loudness.py): only its forced-update equivalent is.
It does not pin lsp-dsp-lib's array primitives or their SIMD variants (dsp::max_index
and dsp::abs_mul3 of the Limiter among them), the order of the Sidechain's refresh sums,
the Lanczos tables or the arithmetic inside an IIR section (the Sidechain's detectors
themselves have been pinned since: _ref/sidechain_ref).
"""
from .binding import *  # noqa: F401,F403
from . import spectral  # noqa: F401,E402
from . import delay  # noqa: F401,E402
from . import equalizer  # noqa: F401,E402
