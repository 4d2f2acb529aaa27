"""ctypes binding of the C ABI declared in include/stochopy_hip.h.

The product path has NO CPU fallback: if the shared library was not built, or
it cannot be loaded, importing a device op raises immediately.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libstochopy_hip.so")

SX_STATUS_NONE = 100
# rows of more than NARROW_DIM elements are "wide" (csrc/sx_wide.hip: one workgroup per row): no chained / peer-exchange /
# ordered-sweep kernels for those, everything else is served; WIDE_DIM is the longest row
# NARROW_DIM is what the wavefront-per-row kernels can serve (the limit of the ordered sweeps, the chained / peer-exchange
# kernels and full CMA-ES); from which length on rows actually TAKE the wide kernels is the library's choice: wide_from()
NARROW_DIM, WIDE_DIM = 4096, 262144


def wide_from():
    """Rows of more than this many elements are served by the one-workgroup-per-row kernels (csrc/sx_device.hpp kWideFrom)."""
    return int(lib().sx_wide_from())
SX_RNG_HOST, SX_RNG_PHILOX = 0, 1

FUN_IDS = {
    "ackley": 0,
    "griewank": 1,
    "quartic": 2,
    "rastrigin": 3,
    "rosenbrock": 4,
    "sphere": 5,
    "styblinski_tang": 6,
}
DE_STRATEGIES = {"rand1bin": 0, "rand2bin": 1, "best1bin": 2, "best2bin": 3}
DE_DONORS = {"rand1bin": 3, "rand2bin": 5, "best1bin": 2, "best2bin": 4}

vp = C.c_void_p
i64 = C.c_int64
i32 = C.c_int32
f64 = C.c_double


class SxState(C.Structure):
    _fields_ = [("it", i64), ("gbidx", i64), ("gfit", f64), ("dx", f64), ("status", i32), ("done", i32),
                ("reserved", i64 * 3)]


class SxDeArgs(C.Structure):
    _fields_ = [
        ("buf0", vp), ("buf1", vp), ("fit", vp), ("candfit", vp), ("gbest", vp), ("lower", vp),
        ("upper", vp), ("state", vp), ("part_f", vp), ("part_i", vp), ("r1", vp), ("donors", vp),
        ("irand", vp), ("resample", vp),
        ("P", i64), ("ld", i64), ("row0", i64),
        ("n", i32), ("fun_id", i32), ("strategy", i32), ("constraints", i32), ("rng", i32), ("maxiter", i32),
        ("wide_from", i32), ("spec_store", i32),
        ("F", f64), ("CR", f64), ("xtol", f64), ("ftol", f64),
        ("key0", C.c_uint32), ("key1", C.c_uint32),
    ]


class SxPsoArgs(C.Structure):
    _fields_ = [
        ("X", vp), ("V", vp), ("pbest", vp), ("pbestfit", vp), ("candfit", vp), ("gbest", vp), ("lower", vp),
        ("upper", vp), ("state", vp), ("part_f", vp), ("part_i", vp), ("r1", vp), ("r2", vp), ("pending_restart", vp),
        ("P", i64), ("ld", i64), ("row0", i64),
        ("n", i32), ("fun_id", i32), ("constraints", i32), ("rng", i32), ("maxiter", i32), ("pad", i32),
        ("w", f64), ("c1", f64), ("c2", f64), ("xtol", f64), ("ftol", f64),
        ("key0", C.c_uint32), ("key1", C.c_uint32),
    ]


SX_MAX_PEERS = 8
SX_IPC_HANDLE_BYTES = 64


class SxXchgArgs(C.Structure):
    _fields_ = [("peer", vp * SX_MAX_PEERS), ("world", i32), ("rank", i32), ("timeout_ticks", i64), ("error", vp),
                ("relay", vp), ("pop0", vp * SX_MAX_PEERS), ("pop1", vp * SX_MAX_PEERS), ("global_rows", i64),
                ("shard_rows", i64)]


class SxCmaState(C.Structure):
    _fields_ = [("it", i64), ("nfev", i64), ("best_row", i64), ("fbest", f64), ("sigma", f64), ("sigma_next", f64),
                ("tmp_coef", f64), ("psnorm", f64), ("status", i32), ("done", i32), ("stop_it", i64),
                ("reserved", f64 * 6)]


class SxVdArgs(C.Structure):
    _fields_ = [
        ("Z", vp), ("ary", vp), ("arx", vp), ("fit", vp), ("xmean", vp), ("xold", vp), ("dx", vp), ("dvec", vp),
        ("vvec", vp), ("vn", vp), ("pc", vp), ("zinj", vp), ("dy", vp), ("w", vp), ("mws", vp), ("mout", vp),
        ("besthist", vp), ("xm", vp), ("xstd", vp), ("xbest", vp), ("hist_x", vp), ("hist_f", vp), ("order", vp),
        ("state", vp), ("pen_ws", vp), ("pen_order", vp), ("P", i64), ("hist_rows", i64),
        ("n", i32), ("mu", i32), ("fun_id", i32), ("maxiter", i32), ("ilim", i32), ("pad", i32),
        ("cs", f64), ("ds", f64), ("cc", f64), ("c1", f64), ("cmu", f64), ("mueff", f64), ("wsum", f64), ("xtol", f64),
        ("ftol", f64), ("insigma", f64), ("key0", C.c_uint32), ("key1", C.c_uint32),
    ]


class SxCmaArgs(C.Structure):
    _fields_ = [
        ("Z", vp), ("arx", vp), ("fit", vp), ("xmean", vp), ("xold", vp), ("ps", vp), ("pc", vp), ("C", vp), ("B", vp),
        ("D", vp), ("eigw", vp), ("w", vp), ("Y", vp), ("part", vp), ("step", vp), ("isc", vp), ("xnew", vp),
        ("ypart", vp), ("besthist", vp), ("xm", vp), ("xstd", vp),
        ("xbest", vp), ("hist_x", vp), ("hist_f", vp), ("order", vp), ("state", vp), ("eigh_ws", vp),
        ("pen_ws", vp), ("pen_order", vp),
        ("eigh_ws_bytes", i64), ("P", i64), ("hist_rows", i64),
        ("n", i32), ("mu", i32), ("fun_id", i32), ("maxiter", i32), ("ilim", i32), ("eig_sweeps", i32),
        ("cs", f64), ("cc", f64), ("c1", f64), ("cmu", f64), ("damps", f64), ("chind", f64), ("mueff", f64),
        ("xtol", f64), ("ftol", f64), ("insigma", f64),
        ("key0", C.c_uint32), ("key1", C.c_uint32),
    ]


SX_SAMPLE_MCMC, SX_SAMPLE_HMC, SX_SAMPLE_ENSEMBLE = 0, 1, 2
SX_JAC_FINITE_DIFF, SX_JAC_ANALYTIC = 0, 1


class SxSampleArgs(C.Structure):
    _fields_ = [
        ("cur", vp), ("fcur", vp), ("facc", vp), ("fmin", vp), ("xbest", vp),
        ("iacc", vp), ("imin", vp), ("nacc", vp), ("nfeas", vp),
        ("x0", vp), ("xall", vp), ("funall", vp), ("lower", vp), ("upper", vp), ("step", vp), ("normals", vp), ("logu", vp),
        ("C", i64), ("x0_stride", i64), ("maxiter", i64),
        ("n", i32), ("fun_id", i32), ("method", i32), ("rng", i32), ("reject", i32), ("k", i32), ("nleap", i32), ("jac", i32),
        ("fd_step", f64),
        ("key0", C.c_uint32), ("key1", C.c_uint32),
    ]


class SxSampleAdapt(C.Structure):
    """sx_sample_adapt: per-chain step-size adaptation in a warm-up, burn-in and thinning (its size is checked against
    sx_sample_adapt_bytes; sx_struct_size is not extended)."""
    _fields_ = [
        ("scale", vp), ("hbar", vp), ("logsbar", vp), ("nacc_warm", vp),
        ("warmup", i64), ("rec_start", i64), ("rec_every", i64), ("rec_rows", i64),
        ("target", f64),
    ]


class SxSampleMetric(C.Structure):
    """sx_sample_metric: per-axis scale adaptation in the warm-up (its size is checked against sx_sample_metric_bytes)."""
    _fields_ = [
        ("sbase", vp), ("m", vp), ("mean", vp), ("M2", vp),
        ("nwin", i32),
        ("win_start", i64), ("win_end", i64 * 8),
    ]


SX_ENSEMBLE_STRETCH, SX_ENSEMBLE_DE, SX_ENSEMBLE_SNOOKER = 0, 1, 2


class SxSampleEnsembleOpts(C.Structure):
    """sx_sample_ensemble_opts: the moves of an ensemble run (kind, running sum of the weights, parameter), its burn-in and
    thinning (its size is checked against sx_sample_ensemble_opts_bytes)."""
    _fields_ = [
        ("nmoves", i32), ("kind", i32 * 4), ("cum", f64 * 4), ("param", f64 * 4),
        ("rec_start", i64), ("rec_every", i64), ("rec_rows", i64),
    ]


class SxSmcArgs(C.Structure):
    """sx_smc_args: tempered sequential Monte Carlo (its size is checked against sx_smc_args_bytes)."""
    _fields_ = [
        ("x", vp * 2), ("f", vp * 2), ("anc", vp), ("nacc", vp), ("step", vp), ("state", vp), ("lower", vp), ("upper", vp),
        ("C", i64), ("P", i64),
        ("n", i32), ("fun_id", i32), ("steps", i32), ("maxiter", i32),
        ("ess", f64), ("target", f64), ("scale", f64),
        ("key0", C.c_uint32), ("key1", C.c_uint32),
    ]


class SxDeRunsArgs(C.Structure):
    _fields_ = [
        ("keys", vp), ("lower", vp), ("upper", vp), ("x0", vp), ("xs", vp), ("funs", vp), ("nits", vp), ("statuses", vp),
        ("xfinal", vp),
        ("R", i64), ("P", i64), ("x0_stride", i64),
        ("n", i32), ("fun_id", i32), ("strategy", i32), ("constraints", i32), ("maxiter", i32), ("pad", i32),
        ("F", f64), ("CR", f64), ("xtol", f64), ("ftol", f64),
    ]


class SxPsoRunsArgs(C.Structure):
    _fields_ = [
        ("keys", vp), ("lower", vp), ("upper", vp), ("x0", vp), ("xs", vp), ("funs", vp), ("nits", vp), ("statuses", vp),
        ("xfinal", vp), ("pbest_final", vp), ("pbestfit_final", vp), ("vwork", vp),
        ("R", i64), ("P", i64), ("x0_stride", i64),
        ("n", i32), ("fun_id", i32), ("constraints", i32), ("maxiter", i32),
        ("w", f64), ("c1", f64), ("c2", f64), ("gamma", f64), ("delta", f64), ("xtol", f64), ("ftol", f64),
    ]


class SxCmaRunsArgs(C.Structure):
    _fields_ = [
        ("keys", vp), ("xmean0", vp), ("xm", vp), ("xstd", vp), ("w", vp), ("work", vp), ("xs", vp), ("funs", vp), ("nits", vp),
        ("statuses", vp), ("nfevs", vp), ("sigmas", vp), ("xmeans", vp),
        ("R", i64), ("P", i64),
        ("n", i32), ("mu", i32), ("fun_id", i32), ("maxiter", i32), ("ilim", i32), ("pad", i32),
        ("mueff", f64), ("cc", f64), ("cs", f64), ("c1", f64), ("cmu", f64), ("damps", f64), ("chind", f64),
        ("sigma", f64), ("insigma", f64), ("xtol", f64), ("ftol", f64),
    ]


class SxVdRunsArgs(C.Structure):
    _fields_ = [
        ("keys", vp), ("xmean0", vp), ("vvec0", vp), ("xm", vp), ("xstd", vp), ("w", vp), ("work", vp), ("xs", vp),
        ("funs", vp), ("nits", vp), ("statuses", vp), ("nfevs", vp), ("sigmas", vp), ("xmeans", vp), ("dvecs", vp),
        ("vvecs", vp),
        ("R", i64), ("P", i64),
        ("n", i32), ("mu", i32), ("fun_id", i32), ("maxiter", i32), ("ilim", i32), ("pad", i32),
        ("mueff", f64), ("cc", f64), ("c1", f64), ("cmu", f64), ("cs", f64), ("ds", f64), ("wsum", f64),
        ("sigma", f64), ("insigma", f64), ("xtol", f64), ("ftol", f64),
    ]


class SxRunsRowwiseArgs(C.Structure):
    _fields_ = [
        ("keys", vp), ("lower", vp), ("upper", vp), ("x0", vp), ("pop0", vp), ("pop1", vp), ("pop2", vp), ("fit", vp),
        ("candfit", vp), ("f", vp), ("state", vp), ("gbest", vp), ("part_f", vp), ("part_i", vp), ("xs", vp), ("funs", vp),
        ("nits", vp), ("statuses", vp), ("ended", vp),
        ("R", i64), ("P", i64), ("x0_stride", i64),
        ("n", i32), ("method", i32), ("strategy", i32), ("constraints", i32), ("maxiter", i32), ("pad", i32),
        ("F", f64), ("CR", f64), ("w", f64), ("c1", f64), ("c2", f64), ("xtol", f64), ("ftol", f64),
    ]


# name -> (restype, argtypes); every symbol include/stochopy_hip.h declares
PROTOTYPES = {
    "sx_abi_version": (C.c_int, []),
    "sx_wide_from": (C.c_int, []),
    "sx_last_error": (C.c_char_p, []),
    "sx_device_count": (C.c_int, []),
    "sx_struct_size": (C.c_int, [C.c_int]),
    "sx_sum_plan": (C.c_int, [i64, vp, C.c_int]),
    "sx_fun_terms": (i64, [C.c_int, C.c_int]),
    "sx_num_partials": (i64, [i64, C.c_int]),
    "sx_de_num_partials": (i64, [i64, C.c_int, C.c_int]),
    "sx_rows_per_workgroup": (C.c_int, [C.c_int]),
    "sx_eval": (C.c_int, [C.c_int, vp, i64, C.c_int, i64, vp, vp, vp, vp, vp, vp]),
    "sx_philox_lhs": (C.c_int, [vp, i64, C.c_int, i64, i64, i64, vp, vp, C.c_uint32, C.c_uint32, vp]),
    "sx_argmin": (C.c_int, [vp, i64, vp, vp, i64, vp, vp, vp]),
    "sx_de_generation": (C.c_int, [C.POINTER(SxDeArgs), C.c_int, vp]),
    "sx_select_finalize": (C.c_int, [vp, vp, i64, vp, vp, i64, C.c_int, vp, vp, C.c_int, f64, f64, vp]),
    "sx_shard_best": (C.c_int, [vp, vp, i64, vp, vp, i64, C.c_int, vp, i64, vp, vp]),
    "sx_gather_finalize": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, C.c_int, f64, f64, vp]),
    "sx_de_shard_generation": (C.c_int, [C.POINTER(SxDeArgs), vp, vp]),
    "sx_de_graph_create": (C.c_int, [C.POINTER(SxDeArgs), C.c_int, C.POINTER(vp)]),
    "sx_de_chain_launch": (C.c_int, [C.POINTER(SxDeArgs), C.c_int, C.c_int, vp]),
    "sx_de_chain_graph_create": (C.c_int, [C.POINTER(SxDeArgs), C.c_int, C.c_int, C.POINTER(vp)]),
    "sx_xchg_bytes": (i64, [C.c_int, C.c_int]),
    "sx_xchg_relay_bytes": (i64, [C.c_int]),
    "sx_xchg_alloc": (C.c_int, [i64, C.POINTER(vp), vp]),
    "sx_xchg_free": (C.c_int, [vp]),
    "sx_pop_alloc": (C.c_int, [i64, C.POINTER(vp), vp]),
    "sx_xchg_open": (C.c_int, [vp, C.POINTER(vp)]),
    "sx_xchg_close": (C.c_int, [vp]),
    "sx_xchg_probe": (C.c_int, [C.POINTER(SxXchgArgs), C.c_int, C.c_int, vp]),
    "sx_xchg_read_record": (C.c_int, [C.POINTER(SxXchgArgs), C.c_int, C.c_int, C.c_int, vp, vp]),
    "sx_xchg_finalize": (C.c_int, [vp, vp, i64, vp, vp, i64, C.c_int, i64, vp, vp, C.c_int, f64, f64,
                                   C.POINTER(SxXchgArgs), vp]),
    "sx_de_p2p_launch": (C.c_int, [C.POINTER(SxDeArgs), C.POINTER(SxXchgArgs), C.c_int, C.c_int, vp]),
    "sx_de_p2p_graph_create": (C.c_int, [C.POINTER(SxDeArgs), C.POINTER(SxXchgArgs), C.c_int, C.c_int,
                                         C.POINTER(vp)]),
    "sx_graph_launch": (C.c_int, [vp, vp]),
    "sx_graph_destroy": (C.c_int, [vp]),
    "sx_pso_generation": (C.c_int, [C.POINTER(SxPsoArgs), C.c_int, vp]),
    "sx_pso_radius": (C.c_int, [C.POINTER(SxPsoArgs), vp, vp]),
    "sx_pso_restart_select": (C.c_int, [C.POINTER(SxPsoArgs), vp, f64, f64, vp, vp]),
    "sx_pso_restart_apply": (C.c_int, [C.POINTER(SxPsoArgs), vp, vp, vp, i64, vp]),
    "sx_pso_restart_select_gathered": (C.c_int, [C.POINTER(SxPsoArgs), vp, C.c_int, f64, f64, vp, vp]),
    "sx_pso_graph_create": (C.c_int, [C.POINTER(SxPsoArgs), C.c_int, vp, f64, f64, vp, C.POINTER(vp)]),
    "sx_de_async_generation": (C.c_int, [C.POINTER(SxDeArgs), vp]),
    "sx_de_propose": (C.c_int, [C.POINTER(SxDeArgs), vp, vp]),
    "sx_pso_move": (C.c_int, [C.POINTER(SxPsoArgs), vp]),
    "sx_rows_select": (C.c_int, [vp, i64, vp, vp, vp, i64, vp, vp, i64, C.c_int, vp, vp, vp, vp]),
    "sx_pso_async_generation": (C.c_int, [C.POINTER(SxPsoArgs), vp]),
    "sx_cmaes_sample": (C.c_int, [vp, f64, vp, vp, vp, vp, i64, C.c_int, vp]),
    "sx_cmaes_recombine": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, vp, vp]),
    "sx_cmaes_rank_mu": (C.c_int, [vp, vp, vp, C.c_int, vp, f64, vp, f64, f64, f64, vp, vp, C.c_int, vp]),
    "sx_cmaes_normals": (C.c_int, [vp, i64, C.c_int, i64, C.c_uint32, C.c_uint32, C.c_uint32, vp]),
    "sx_symmetrize_upper": (C.c_int, [vp, C.c_int, vp]),
    "sx_cmaes_eval_penalized": (C.c_int, [C.c_int, vp, i64, C.c_int, vp, vp, vp, vp, vp, vp]),
    "sx_vdcma_sample": (C.c_int, [vp, i64, C.c_int, i64, vp, vp, f64, vp, f64, vp, vp, vp, vp]),
    "sx_na_blocks": (C.c_int, [i64]),
    "sx_na_begin": (C.c_int, [vp, i64, i64, C.c_int, vp, i64, vp, vp, vp]),
    "sx_na_axis": (C.c_int, [vp, i64, i64, C.c_int, C.c_int, C.c_int, vp, i64, vp, vp, vp, vp, vp, vp, vp]),
    "sx_na_commit": (C.c_int, [vp, i64, C.c_int, vp, vp, i64, i64, vp]),
    "sx_na_uniforms": (C.c_int, [vp, i64, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, vp]),
    "sx_vdcma_moments": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, f64, vp, vp, vp]),
    "sx_cmaes_generation": (C.c_int, [C.POINTER(SxCmaArgs), i64, C.c_int, vp]),
    "sx_cma_rank": (C.c_int, [vp, i64, vp, vp, vp, i64, vp]),
    "sx_cma_penalize": (C.c_int, [C.POINTER(SxCmaArgs), i64, vp, vp, vp]),
    "sx_cmaes_generation_stage": (C.c_int, [C.POINTER(SxCmaArgs), i64, C.c_int, C.c_int, i64, i64, vp, vp, vp]),
    "sx_cmaes_generation_phased": (C.c_int, [C.POINTER(SxCmaArgs), i64, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "sx_eigh_rounds_per_sweep": (C.c_int, [C.c_int]),
    "sx_vdcma_generation": (C.c_int, [C.POINTER(SxVdArgs), i64, vp]),
    "sx_vdcma_generation_stage": (C.c_int, [C.POINTER(SxVdArgs), i64, C.c_int, i64, i64, vp, vp, vp, vp]),
    "sx_eigh_workspace_bytes": (i64, [C.c_int]),
    "sx_eigh": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, i64, C.c_int, f64, vp]),
    "sx_eigh_refined": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, i64, C.c_int, f64, C.c_int, vp]),
    "sx_eigh_info": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(f64), vp]),
    "sx_sample_run": (C.c_int, [C.POINTER(SxSampleArgs), i64, i64, vp]),
    "sx_sample_chains_per_workgroup": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "sx_sample_gradient": (C.c_int, [C.c_int, vp, i64, C.c_int, vp, vp]),
    "sx_sample_propose": (C.c_int, [C.POINTER(SxSampleArgs), i64, vp, vp, vp, vp]),
    "sx_sample_leap": (C.c_int, [C.POINTER(SxSampleArgs), f64, C.c_int, vp, vp, vp, vp]),
    "sx_sample_fd_rows": (C.c_int, [C.POINTER(SxSampleArgs), vp, C.c_int, C.c_int, vp, vp]),
    "sx_sample_fd_gradient": (C.c_int, [C.POINTER(SxSampleArgs), vp, C.c_int, C.c_int, vp, vp]),
    "sx_sample_decide": (C.c_int, [C.POINTER(SxSampleArgs), i64, vp, vp, vp, vp, vp]),
    "sx_sample_adapt_bytes": (C.c_int, []),
    "sx_sample_run_adapt": (C.c_int, [C.POINTER(SxSampleArgs), C.POINTER(SxSampleAdapt), i64, i64, vp]),
    "sx_sample_propose_adapt": (C.c_int, [C.POINTER(SxSampleArgs), C.POINTER(SxSampleAdapt), i64, vp, vp, vp, vp]),
    "sx_sample_leap_adapt": (C.c_int, [C.POINTER(SxSampleArgs), C.POINTER(SxSampleAdapt), f64, C.c_int, vp, vp, vp, vp]),
    "sx_sample_decide_adapt": (C.c_int, [C.POINTER(SxSampleArgs), C.POINTER(SxSampleAdapt), i64, vp, vp, vp, vp, vp]),
    "sx_sample_metric_bytes": (C.c_int, []),
    "sx_sample_run_metric": (C.c_int, [C.POINTER(SxSampleArgs), C.POINTER(SxSampleAdapt), C.POINTER(SxSampleMetric), i64, i64, vp]),
    "sx_sample_propose_metric": (C.c_int, [C.POINTER(SxSampleArgs), C.POINTER(SxSampleAdapt), C.POINTER(SxSampleMetric), i64, vp, vp,
                                           vp, vp]),
    "sx_sample_leap_metric": (C.c_int, [C.POINTER(SxSampleArgs), C.POINTER(SxSampleAdapt), C.POINTER(SxSampleMetric), f64, C.c_int,
                                        vp, vp, vp, vp]),
    "sx_sample_decide_metric": (C.c_int, [C.POINTER(SxSampleArgs), C.POINTER(SxSampleAdapt), C.POINTER(SxSampleMetric), i64, vp, vp,
                                          vp, vp, vp]),
    "sx_sample_tempered_run": (C.c_int, [C.POINTER(SxSampleArgs), vp, C.c_int, i64, vp, i64, i64, vp]),
    "sx_sample_tempered_max_rungs": (C.c_int, [C.c_int]),
    "sx_sample_decide_tempered": (C.c_int, [C.POINTER(SxSampleArgs), i64, vp, vp, vp, C.c_int, C.c_int, vp]),
    "sx_sample_swap": (C.c_int, [C.POINTER(SxSampleArgs), i64, i64, vp, C.c_int, vp, vp]),
    "sx_sample_ensemble_run": (C.c_int, [C.POINTER(SxSampleArgs), C.c_int, f64, i64, i64, vp]),
    "sx_sample_ensemble_lds_bytes": (C.c_int, [C.c_int, C.c_int]),
    "sx_sample_ensemble_propose": (C.c_int, [C.POINTER(SxSampleArgs), C.c_int, f64, i64, C.c_int, vp, vp, vp]),
    "sx_sample_ensemble_decide": (C.c_int, [C.POINTER(SxSampleArgs), C.c_int, i64, C.c_int, vp, vp, vp, vp]),
    "sx_sample_ensemble_opts_bytes": (C.c_int, []),
    "sx_sample_ensemble_run_moves": (C.c_int, [C.POINTER(SxSampleArgs), C.c_int, C.POINTER(SxSampleEnsembleOpts), i64, i64, vp]),
    "sx_sample_ensemble_propose_moves": (C.c_int, [C.POINTER(SxSampleArgs), C.c_int, C.POINTER(SxSampleEnsembleOpts), i64, C.c_int,
                                                   vp, vp, vp]),
    "sx_sample_ensemble_decide_moves": (C.c_int, [C.POINTER(SxSampleArgs), C.c_int, C.POINTER(SxSampleEnsembleOpts), i64, C.c_int,
                                                  vp, vp, vp, vp]),
    "sx_smc_args_bytes": (C.c_int, []),
    "sx_smc_max_particles": (C.c_int, []),
    "sx_smc_init": (C.c_int, [C.POINTER(SxSmcArgs), vp]),
    "sx_smc_stage": (C.c_int, [C.POINTER(SxSmcArgs), C.c_int, vp]),
    "sx_smc_resample": (C.c_int, [C.POINTER(SxSmcArgs), C.c_int, vp]),
    "sx_smc_mutate": (C.c_int, [C.POINTER(SxSmcArgs), C.c_int, vp]),
    "sx_smc_propose": (C.c_int, [C.POINTER(SxSmcArgs), C.c_int, C.c_int, vp, vp]),
    "sx_smc_decide": (C.c_int, [C.POINTER(SxSmcArgs), C.c_int, C.c_int, vp, vp, vp]),
    "sx_de_runs_launch": (C.c_int, [C.POINTER(SxDeRunsArgs), vp]),
    "sx_de_runs_sweep_launch": (C.c_int, [C.POINTER(SxDeRunsArgs), vp, vp, vp, vp]),
    "sx_de_runs_lds_bytes": (i64, [i64, C.c_int]),
    "sx_pso_runs_launch": (C.c_int, [C.POINTER(SxPsoRunsArgs), vp]),
    "sx_pso_runs_sweep_launch": (C.c_int, [C.POINTER(SxPsoRunsArgs), vp, vp, vp, vp, vp]),
    "sx_pso_runs_lds_bytes": (i64, [i64, C.c_int]),
    "sx_pso_runs_workspace_bytes": (i64, [i64, i64, C.c_int]),
    "sx_cma_runs_launch": (C.c_int, [C.POINTER(SxCmaRunsArgs), vp]),
    "sx_cma_runs_sweep_launch": (C.c_int, [C.POINTER(SxCmaRunsArgs), vp, vp]),
    "sx_cma_runs_lds_bytes": (i64, [i64, C.c_int]),
    "sx_cma_runs_workspace_bytes": (i64, [i64, i64]),
    "sx_vd_runs_launch": (C.c_int, [C.POINTER(SxVdRunsArgs), vp]),
    "sx_vd_runs_sweep_launch": (C.c_int, [C.POINTER(SxVdRunsArgs), vp, vp]),
    "sx_vd_runs_args_bytes": (C.c_int, []),
    "sx_vd_runs_lds_bytes": (i64, [i64, C.c_int]),
    "sx_vd_runs_workspace_bytes": (i64, [i64, i64]),
    "sx_runs_rowwise_partials": (i64, [i64, C.c_int]),
    "sx_runs_rowwise_init": (C.c_int, [C.POINTER(SxRunsRowwiseArgs), vp]),
    "sx_runs_rowwise_start": (C.c_int, [C.POINTER(SxRunsRowwiseArgs), vp, vp]),
    "sx_runs_rowwise_de_propose": (C.c_int, [C.POINTER(SxRunsRowwiseArgs), vp, vp, vp, vp]),
    "sx_runs_rowwise_pso_move": (C.c_int, [C.POINTER(SxRunsRowwiseArgs), vp, vp, vp, vp]),
    "sx_runs_rowwise_select": (C.c_int, [C.POINTER(SxRunsRowwiseArgs), vp]),
    "sx_runs_rowwise_finalize": (C.c_int, [C.POINTER(SxRunsRowwiseArgs), vp]),
    "sx_mt_create": (vp, [C.c_uint32]),
    "sx_mt_destroy": (None, [vp]),
    "sx_mt_seed": (None, [vp, C.c_uint32]),
    "sx_mt_random": (None, [vp, vp, i64]),
    "sx_mt_uniform": (None, [vp, f64, f64, vp, i64]),
    "sx_mt_uniform_rows": (None, [vp, vp, vp, C.c_int, i64, vp]),
    "sx_mt_randn": (None, [vp, vp, i64]),
    "sx_mt_randint": (None, [vp, i64, vp, i64]),
    "sx_mt_permutation": (None, [vp, i64, vp]),
    "sx_mt_latin_hypercube": (None, [vp, i64, C.c_int, vp, vp, vp, vp]),
    "sx_mt_de_donors": (None, [vp, i64, C.c_int, vp]),
    "sx_mt_de_async_draws": (None, [vp, i64, C.c_int, C.c_int, vp, vp, vp, vp, vp]),
    "sx_mt_get_state": (None, [vp, vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(f64)]),
    "sx_mt_set_state": (None, [vp, vp, C.c_int, C.c_int, f64]),
}

_lib = None


class HipLibraryError(RuntimeError):
    pass


def lib():
    """Load the HIP library (once).  Raises HipLibraryError if it is missing -- never falls back."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipLibraryError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C stochopy_amd/csrc`.  stochopy_amd has no CPU fallback.")
    try:
        handle = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    except OSError as e:  # pragma: no cover
        raise HipLibraryError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in PROTOTYPES.items():
        try:
            fn = getattr(handle, name)
        except AttributeError as e:
            raise HipLibraryError(f"{LIB_PATH} does not export {name}; rebuild it") from e
        fn.restype = res
        fn.argtypes = args
    if handle.sx_abi_version() != 1:
        raise HipLibraryError("ABI version mismatch; rebuild the library")
    for which, mirror in enumerate((SxState, SxDeArgs, SxPsoArgs, SxXchgArgs, SxCmaState, SxCmaArgs, SxVdArgs,
                                    SxSampleArgs, SxDeRunsArgs, SxPsoRunsArgs, SxCmaRunsArgs, None, SxRunsRowwiseArgs)):
        if mirror is None:  # (11: no struct; sx_vd_runs_args has sx_vd_runs_args_bytes, below)
            continue
        if handle.sx_struct_size(which) != C.sizeof(mirror):  # (a library built against another layout of the structs)
            raise HipLibraryError(f"{LIB_PATH}: struct {which} is {handle.sx_struct_size(which)} bytes, its mirror "
                                  f"{C.sizeof(mirror)}; rebuild the library")
    if handle.sx_vd_runs_args_bytes() != C.sizeof(SxVdRunsArgs):
        raise HipLibraryError(f"{LIB_PATH}: sx_vd_runs_args is {handle.sx_vd_runs_args_bytes()} bytes, its mirror "
                              f"{C.sizeof(SxVdRunsArgs)}; rebuild the library")
    if handle.sx_sample_adapt_bytes() != C.sizeof(SxSampleAdapt):
        raise HipLibraryError(f"{LIB_PATH}: sx_sample_adapt is {handle.sx_sample_adapt_bytes()} bytes, its mirror "
                              f"{C.sizeof(SxSampleAdapt)}; rebuild the library")
    if handle.sx_sample_metric_bytes() != C.sizeof(SxSampleMetric):
        raise HipLibraryError(f"{LIB_PATH}: sx_sample_metric is {handle.sx_sample_metric_bytes()} bytes, its mirror "
                              f"{C.sizeof(SxSampleMetric)}; rebuild the library")
    if handle.sx_sample_ensemble_opts_bytes() != C.sizeof(SxSampleEnsembleOpts):
        raise HipLibraryError(f"{LIB_PATH}: sx_sample_ensemble_opts is {handle.sx_sample_ensemble_opts_bytes()} bytes, its mirror "
                              f"{C.sizeof(SxSampleEnsembleOpts)}; rebuild the library")
    if handle.sx_smc_args_bytes() != C.sizeof(SxSmcArgs):
        raise HipLibraryError(f"{LIB_PATH}: sx_smc_args is {handle.sx_smc_args_bytes()} bytes, its mirror "
                              f"{C.sizeof(SxSmcArgs)}; rebuild the library")
    _lib = handle
    return _lib


def check(rc, what=""):
    if rc != 0:
        raise HipLibraryError(f"{what} failed (rc={rc}): {lib().sx_last_error().decode()}")
