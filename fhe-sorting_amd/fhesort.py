"""Python binding of the MI355X engine (lib/libfhesort.so, C ABI in
include/fhe_gpu.h).

This is the host-side handle the tests and bench.py use.  There is no CPU
fallback: if the HIP library is missing or no GPU is visible, constructing a
Context raises.  Method names mirror the reference API where one exists
(compare, indicator, sign_composite, direct_sort, ...).
"""
import contextlib
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('FHE_LIB') or os.path.join(HERE, 'lib', 'libfhesort.so')  # FHE_LIB: A/B builds
COEFF_DIR = os.path.join(HERE, 'data')
HEADER = os.path.join(os.path.dirname(HERE), 'include', 'fhe_gpu.h')
PS_SPLIT_ENGINE, PS_SPLIT_OPENFHE = 0, 1  # fhe_set_ps_split (include/fhe_gpu.h)
RUN_ROWS, RUN_LE, RUN_LT, RUN_BETWEEN = range(4)  # fhe_direct_running_sum's modes (FHE_RUN_*)
WIN_ROWS, WIN_LE, WIN_LT, WIN_BETWEEN, WIN_GROUP = range(5)  # fhe_direct_window_sum's modes (FHE_WIN_*)

FHE_OK, FHE_EINVAL, FHE_ENOKEY, FHE_EDEPTH, FHE_EHIP, FHE_ENOMEM, FHE_EINTERNAL, FHE_ENOCOMM, FHE_EIO = range(9)
NAF, BNAF, BINARY = 0, 1, 2
SORT_COLUMN_MEMBERS_DEFAULT = 256  # fhe_set_sort_column_members' initial value (csrc/capi/capi.cpp)
TENSOR_COLS_PER_THREAD = 4         # columns a k_tensor_cols thread owns (TC_PC, csrc/device/kernels.hip)
PLAIN_SUM_GROUPS_PER_THREAD = 4    # groups a k_mul_plain_sum_groups thread owns (PSG_TG, csrc/device/kernels.hip)


class FheError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f'fhe error {code}: {msg}')
        self.code = code


class NoKeyError(FheError):
    pass


class Params(C.Structure):
    _fields_ = [('log_n', C.c_int), ('mult_depth', C.c_int), ('scale_bits', C.c_int), ('first_bits', C.c_int),
                ('dnum', C.c_int), ('seed', C.c_uint64)]


_lib = None
vp, ip, dp, u64p = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_uint64)
PP = C.POINTER(C.c_void_p)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_uint64), C.c_uint64, C.c_void_p)


class _Hook:
    """ctypes wrapper of a Python all-reduce callback f(dev_ptr, count, user):
    an exception inside it is recorded and reported as a non-zero return (the
    C side then aborts the sort); the caller re-raises it after the C call."""

    def __init__(self, f):
        self.exc = None

        def call(ptr, count, user):
            try:
                r = f(ptr, count, user)
                return 0 if r is None else int(r)
            except BaseException as e:  # noqa: BLE001 -- must not unwind through C
                self.exc = e
                return 1
        self.fn = ALLREDUCE_FN(call) if f else None

    def ptr(self):
        return C.cast(self.fn, C.c_void_p) if self.fn else None

    def reraise(self, err):
        if self.exc is not None:
            raise self.exc from err
        raise err

_SIGS = {
    'fhe_last_error': (C.c_char_p, []),
    'fhe_params_check': (C.c_int, [C.POINTER(Params), ip, ip, ip, ip]),
    'fhe_ctx_create': (C.c_int, [C.POINTER(Params), C.c_int, PP]),
    'fhe_ctx_destroy': (C.c_int, [vp]),
    'fhe_ctx_info': (C.c_int, [vp, ip, ip, ip, u64p, dp]),
    'fhe_set_coeff_dir': (C.c_int, [C.c_char_p]),
    'fhe_keygen': (C.c_int, [vp]),
    'fhe_gen_rotation_keys': (C.c_int, [vp, ip, C.c_int]),
    'fhe_ctx_load_secret': (C.c_int, [vp, u64p]),
    'fhe_ctx_load_public': (C.c_int, [vp, u64p]),
    'fhe_ctx_load_keys': (C.c_int, [vp, u64p, ip, C.POINTER(u64p), C.c_int]),
    'fhe_key_bytes': (C.c_uint64, [vp]),
    'fhe_encrypt': (C.c_int, [vp, dp, C.c_int, C.c_int, C.c_int, PP]),
    'fhe_encrypt_ext': (C.c_int, [vp, dp, C.c_int, C.c_int, PP]),
    'fhe_decrypt': (C.c_int, [vp, vp, dp]),
    'fhe_ct_upload': (C.c_int, [vp, u64p, C.c_int, C.c_int, C.c_int, C.c_double, PP]),
    'fhe_ct_download': (C.c_int, [vp, vp, u64p]),
    'fhe_ct_info': (C.c_int, [vp, ip, ip, dp, ip]),
    'fhe_ct_set_slots': (C.c_int, [vp, C.c_int]),
    'fhe_ct_free': (C.c_int, [vp]),
    'fhe_pt_encode': (C.c_int, [vp, dp, C.c_int, C.c_int, C.c_int, PP]),
    'fhe_pt_upload': (C.c_int, [vp, u64p, C.c_int, C.c_int, C.c_int, C.c_double, PP]),
    'fhe_pt_free': (C.c_int, [vp]),
    'fhe_add': (C.c_int, [vp, vp, vp, PP]),
    'fhe_sub': (C.c_int, [vp, vp, vp, PP]),
    'fhe_negate': (C.c_int, [vp, vp, PP]),
    'fhe_add_const': (C.c_int, [vp, vp, C.c_double, PP]),
    'fhe_mul_const': (C.c_int, [vp, vp, C.c_double, PP]),
    'fhe_mul_const_to': (C.c_int, [vp, vp, C.c_double, C.c_int, PP]),
    'fhe_mul_int': (C.c_int, [vp, vp, C.c_int64, PP]),
    'fhe_level_adjust': (C.c_int, [vp, vp, C.c_int, PP]),
    'fhe_rescale': (C.c_int, [vp, vp, PP]),
    'fhe_mul_plain': (C.c_int, [vp, vp, vp, PP]),
    'fhe_add_plain': (C.c_int, [vp, vp, vp, PP]),
    'fhe_mul_relin': (C.c_int, [vp, vp, vp, PP]),
    'fhe_square_relin': (C.c_int, [vp, vp, PP]),
    'fhe_mul_add': (C.c_int, [vp, vp, vp, PP, dp, C.c_int, vp, vp, PP]),
    'fhe_mul_add_const': (C.c_int, [vp, vp, vp, PP, dp, C.c_int, vp, vp, C.c_double, C.c_double, PP]),
    'fhe_mul_fold_left': (C.c_int, [C.c_int, C.c_int, C.c_int]),
    'fhe_rotate': (C.c_int, [vp, vp, C.c_int, PP]),
    'fhe_rotate_hoisted': (C.c_int, [vp, vp, ip, C.c_int, PP]),
    'fhe_linear_sum_to': (C.c_int, [vp, PP, dp, C.c_int, C.c_int, PP]),
    'fhe_cheb_ps': (C.c_int, [vp, vp, dp, C.c_int, C.c_double, C.c_double, PP]),
    'fhe_sign_composite': (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, PP]),
    'fhe_compare': (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, PP]),
    'fhe_indicator': (C.c_int, [vp, vp, C.c_double, C.c_int, C.c_int, C.c_int, PP]),
    'fhe_compose_rotate': (C.c_int, [vp, vp, C.c_int, ip, C.c_int, C.c_int, C.c_int, PP]),
    'fhe_compose_rotate_members': (C.c_int, [vp, vp, C.c_int, ip, C.c_int, C.c_int, ip, C.c_int, PP]),
    'fhe_decompose': (C.c_int, [C.c_int, ip, C.c_int, C.c_int, C.c_int, C.c_int, ip, ip, C.c_int]),
    'fhe_rotation_tree_create': (C.c_int, [vp, C.c_int, ip, C.c_int, C.c_int, PP]),
    'fhe_rotation_tree_build': (C.c_int, [vp, C.c_int, C.c_int]),
    'fhe_rotation_tree_rotate': (C.c_int, [vp, vp, C.c_int, PP]),
    'fhe_rotation_tree_stats': (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    'fhe_rotation_tree_destroy': (None, [vp]),
    'fhe_size_parameters': (C.c_int, [C.c_int, ip, ip, C.c_int]),
    'fhe_direct_sort': (C.c_int, [vp, vp, vp, C.c_int, ip, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.c_int, C.c_int, vp, vp, PP]),
    'fhe_direct_sort_columns': (C.c_int, [vp, vp, vp, C.POINTER(C.c_void_p), C.c_int, C.c_int, ip, C.c_int, C.c_int,
                                          C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.POINTER(C.c_void_p)]),
    'fhe_set_sort_column_members': (C.c_int, [vp, C.c_int]),
    'fhe_mul_columns': (C.c_int, [vp, vp, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p)]),
    'fhe_ct_sum_member_groups': (C.c_int, [vp, vp, C.c_int, C.POINTER(C.c_void_p)]),
    'fhe_direct_select': (C.c_int, [vp, vp, vp, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int,
                                    ip, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    'fhe_select_layout': (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int]),
    'fhe_pt_encode_select': (C.c_int, [vp, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       PP]),
    'fhe_mul_plain_sum_groups': (C.c_int, [vp, vp, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    'fhe_set_sort_tiebreak': (C.c_int, [vp, C.c_double]),
    'fhe_tiebreak_offsets': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_double, dp]),
    'fhe_set_pair_tables': (C.c_int, [vp, C.c_int, C.c_int]),
    'fhe_pair_shape': (C.c_int, [C.c_int, C.c_int, C.c_int, ip, ip, ip, ip, ip]),
    'fhe_pt_encode_tiebreak': (C.c_int, [vp, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_double, C.c_int,
                                         C.POINTER(C.c_void_p)]),
    'fhe_sub_add_plain_stacked': (C.c_int, [vp, vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int,
                                            C.POINTER(C.c_void_p)]),
    'fhe_direct_group_sum': (C.c_int, [vp, vp, vp, C.POINTER(C.c_void_p), C.c_int, C.c_double, C.c_int, ip, C.c_int,
                                       C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    'fhe_group_sum_levels': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, ip, ip]),
    'fhe_sub_pm_const_stacked': (C.c_int, [vp, vp, C.POINTER(C.c_void_p), C.c_int, C.c_double,
                                           C.POINTER(C.c_void_p)]),
    'fhe_mul_pairs': (C.c_int, [vp, vp, vp, vp, C.c_int, C.POINTER(C.c_void_p)]),
    'fhe_direct_gather': (C.c_int, [vp, vp, vp, C.POINTER(C.c_void_p), C.c_int, ip, C.c_int, C.c_int, C.c_int, C.c_int,
                                    ip, C.c_int, C.POINTER(C.c_void_p)]),
    'fhe_gather_levels': (C.c_int, [C.c_int, C.c_int, ip, ip, ip]),
    'fhe_sub_offsets_stacked': (C.c_int, [vp, vp, C.POINTER(C.c_void_p), C.c_int, ip, C.c_int,
                                          C.POINTER(C.c_void_p)]),
    'fhe_mul_gather': (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    'fhe_direct_running_sum': (C.c_int, [vp, vp, vp, vp, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_double, C.c_int,
                                         ip, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_void_p)]),
    'fhe_sub_bounds_stacked': (C.c_int, [vp, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p), C.c_int, dp,
                                         C.POINTER(C.c_void_p)]),
    'fhe_mul_pairs_const': (C.c_int, [vp, vp, C.c_double, vp, C.c_int, C.POINTER(C.c_void_p)]),
    'fhe_mul_pairs_sub': (C.c_int, [vp, vp, vp, vp, C.c_int, C.POINTER(C.c_void_p)]),
    'fhe_direct_lex_rank': (C.c_int, [vp, C.POINTER(C.c_void_p), C.c_int, C.c_double, C.c_int, ip, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    'fhe_lex_rank_levels': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, ip]),
    'fhe_sub_lex_stacked': (C.c_int, [vp, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p), C.c_int,
                                      C.POINTER(C.c_void_p), C.c_double, C.POINTER(C.c_void_p)]),
    'fhe_mul_lex': (C.c_int, [vp, vp, C.c_double, vp, vp, C.POINTER(C.c_void_p)]),
    'fhe_direct_window_sum': (C.c_int, [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, vp, vp, vp,
                                        C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_double, C.c_int, ip, C.c_int,
                                        C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    'fhe_window_sum_levels': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, ip, ip]),
    'fhe_sub_window_stacked': (C.c_int, [vp, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p), C.c_int, C.c_int,
                                         vp, vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_double,
                                         C.POINTER(C.c_void_p)]),
    'fhe_mul_sub_sub': (C.c_int, [vp, vp, vp, vp, vp, C.POINTER(C.c_void_p)]),
    'fhe_sort_hybrid': (C.c_int, [vp, vp, vp, C.c_int, ip, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.c_int, C.c_int, C.c_int, vp, vp, PP]),
    'fhe_hybrid_parameters': (C.c_int, [C.c_int, ip, ip, C.c_int]),
    'fhe_mehp24_parameters': (C.c_int, [C.c_int, ip, ip, ip, ip, ip, ip, ip, ip, ip, C.c_int]),
    'fhe_mehp24_rotation_indices': (C.c_int, [C.c_int, C.c_int, ip, C.c_int]),
    'fhe_mehp24_sort': (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, PP]),
    'fhe_mehp24_sort_sharded': (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_int, C.c_int, vp, vp, PP]),
    'fhe_mehp24_indicator': (C.c_int, [vp, vp, C.c_double, C.c_int, C.c_int, PP]),
    'fhe_kway_sort': (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, PP]),
    'fhe_kway_sorter': (C.c_int, [vp, C.c_int, PP, C.c_int, PP, C.c_int, PP]),
    'fhe_kway_sort_boot': (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.POINTER(C.c_int), PP]),
    'fhe_boot_create': (C.c_int, [vp, vp, PP]),
    'fhe_boot_destroy': (C.c_int, [vp]),
    'fhe_boot_keygen': (C.c_int, [vp]),
    'fhe_boot_rotation_indices': (C.c_int, [vp, C.POINTER(C.c_int32), C.c_int]),
    'fhe_boot_depth': (C.c_int, [vp]),
    'fhe_bootstrap': (C.c_int, [vp, vp, PP]),
    'fhe_check_level_and_boot': (C.c_int, [vp, vp, C.c_int, vp, C.POINTER(C.c_int), PP]),
    'fhe_bootstrap_stage': (C.c_int, [vp, vp, C.c_int, PP]),
    'fhe_conjugate': (C.c_int, [vp, vp, PP]),
    'fhe_gen_galois_keys': (C.c_int, [vp, u64p, C.c_int]),
    'fhe_ctx_load_galois_key': (C.c_int, [vp, C.c_uint64, u64p]),
    'fhe_pt_encode_complex': (C.c_int, [vp, dp, dp, C.c_int, C.c_int, C.c_int, C.c_double, PP]),
    'fhe_kway_sort_type': (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                     C.POINTER(C.c_int)]),
    'fhe_kway_stage_count': (C.c_int, [C.c_int, C.c_int]),
    'fhe_kway_rotate_distance': (C.c_int, [C.c_int, C.c_int, C.c_int]),
    'fhe_kway_gen_indices': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    'fhe_kway_rotation_indices': (C.c_int, [C.c_int, C.POINTER(C.c_int32), C.c_int]),
    'fhe_comm_get_unique_id': (C.c_int, [C.POINTER(C.c_uint8)]),
    'fhe_comm_init': (C.c_int, [vp, C.POINTER(C.c_uint8), C.c_int, C.c_int]),
    'fhe_comm_destroy': (C.c_int, [vp]),
    'fhe_ct_allreduce': (C.c_int, [vp, vp]),
    'fhe_ntt': (C.c_int, [vp, u64p, C.c_int, C.c_int, C.c_int]),
    'fhe_modup': (C.c_int, [vp, u64p, C.c_int, u64p]),
    'fhe_moddown': (C.c_int, [vp, u64p, C.c_int, u64p]),
    'fhe_automorph': (C.c_int, [vp, u64p, C.c_int, C.c_uint64, u64p]),
    'fhe_linear_sums_raw': (C.c_int, [vp, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_uint8),
                                      C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_uint8), C.c_int,
                                      C.POINTER(C.c_void_p)]),
    'fhe_counters': (C.c_int, [vp, u64p]),
    'fhe_collective_stats': (C.c_int, [vp, u64p]),
    'fhe_boot_counters': (C.c_int, [vp, u64p]),
    'fhe_set_kway_stack': (C.c_int, [vp, C.c_int]),
    'fhe_region_marker': (C.c_int, [vp, C.c_int]),
    'fhe_set_mask_cache': (C.c_int, [vp, C.c_int]),
    'fhe_pt_limbs': (C.c_int, [vp]),
    'fhe_pt_download': (C.c_int, [vp, vp, u64p]),
    'fhe_pt_encode_device': (C.c_int, [vp, dp, C.c_int, C.c_int, C.c_int, PP]),
    'fhe_pt_encode_masks': (C.c_int, [vp, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, PP]),
    'fhe_reset_counters': (C.c_int, [vp]),
    'fhe_sync': (C.c_int, [vp]),
    'fhe_stream': (vp, [vp]),
    'fhe_time_kernel': (C.c_int, [vp, C.c_char_p, C.c_int, C.c_int, dp, dp]),
    'fhe_kernel_clock_start': (C.c_int, [vp]),
    'fhe_set_sort_stack': (C.c_int, [vp, C.c_int]),
    'fhe_set_sort_lanes': (C.c_int, [vp, C.c_int]),
    'fhe_set_ps_split': (C.c_int, [vp, C.c_int]),
    'fhe_ntt_dev': (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int, vp]),
    'fhe_automorph_dev': (C.c_int, [vp, vp, C.c_int, C.c_uint64, vp, vp]),
    'fhe_host_stats': (C.c_int, [dp]),
    'fhe_set_mfma_sums': (C.c_int, [C.c_int]),
    'fhe_host_stats_reset': (C.c_int, []),
    'fhe_prng_block': (C.c_int, [C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    'fhe_get_ps_split': (C.c_int, [vp]),
    'fhe_cheb_ps_depth': (C.c_int, [C.c_int, C.c_int]),
    'fhe_cheb_ps_plan': (C.c_int, [C.POINTER(C.c_double), C.c_int]),
    'fhe_pool_trim': (C.c_int, [vp]),
    'fhe_pool_stats': (C.c_int, [vp, u64p, u64p, u64p]),
    'fhe_ct_stack': (C.c_int, [vp, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p)]),
    'fhe_mul_plain_sum': (C.c_int, [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int,
                                    C.POINTER(C.c_void_p)]),
    'fhe_mul_plain_sum_batches': (C.c_int, [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.c_int,
                                            C.POINTER(C.c_void_p)]),
    'fhe_plain_sum_tile': (C.c_int, []),
    'fhe_plain_sum_batches_limb_units': (C.c_double, [C.c_int, C.c_int, C.c_int]),
    'fhe_ct_member': (C.c_int, [vp, vp, C.c_int, C.POINTER(C.c_void_p)]),
    'fhe_ct_sum_members': (C.c_int, [vp, vp, C.POINTER(C.c_void_p)]),
    'fhe_kernel_clock_stop': (C.c_int, [vp, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    'fhe_wire_inspect': (C.c_int, [C.c_char_p, vp]),
    'fhe_serialize_context': (C.c_int, [vp, C.c_char_p]),
    'fhe_deserialize_context': (C.c_int, [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]),
    'fhe_serialize_ciphertext': (C.c_int, [vp, vp, C.c_char_p]),
    'fhe_deserialize_ciphertext': (C.c_int, [vp, C.c_char_p, C.POINTER(C.c_void_p)]),
    'fhe_deserialize_eval_automorphism_key': (C.c_int, [vp, C.c_char_p, C.POINTER(C.c_int)]),
    **{f'fhe_{d}serialize_{k}': (C.c_int, [vp, C.c_char_p])
       for d in ('', 'de') for k in ('public_key', 'secret_key', 'eval_mult_key')},
    'fhe_serialize_eval_automorphism_key': (C.c_int, [vp, C.c_char_p]),
    'fhe_serialize_eval_mult_key_seeded': (C.c_int, [vp, C.c_char_p]),
    'fhe_serialize_eval_automorphism_key_seeded': (C.c_int, [vp, C.c_char_p]),
    'fhe_set_public_seed': (C.c_int, [vp, C.c_char_p]),
    'fhe_get_public_seed': (C.c_int, [vp, C.c_char_p]),
    'fhe_key_is_seeded': (C.c_int, [vp, C.c_uint64]),
    'fhe_public_poly': (C.c_int, [vp, C.c_char_p, C.c_uint64, C.c_int, u64p]),
}


class WireInfo(C.Structure):
    _fields_ = [('kind', C.c_uint32), ('version', C.c_uint32), ('params_id', C.c_uint64), ('log_n', C.c_uint64),
                ('nq', C.c_uint64), ('K', C.c_uint64), ('body_words', C.c_uint64)]


WIRE_KINDS = {1: 'context', 2: 'public_key', 3: 'eval_mult_key', 4: 'eval_automorphism_key', 5: 'ciphertext',
              6: 'secret_key', 7: 'eval_mult_key_seeded', 8: 'eval_automorphism_key_seeded'}


def set_mfma_sums(mask):
    """Process-wide choice of the i8-MFMA sums-of-products kernels (1 PS linear
    sums, 2 ModUp, 4 ModDown+rescale; fhe_set_mfma_sums).  mask < 0 only
    queries.  Returns the previous mask.  The output words do not change."""
    return lib().fhe_set_mfma_sums(int(mask))


def wire_inspect(path):
    """Header of a wire file (csrc/wire/wire.hpp) after its checksum is verified;
    host only, no GPU needed."""
    i = WireInfo()
    _chk(lib().fhe_wire_inspect(os.fsencode(path), C.byref(i)))
    return {'kind': WIRE_KINDS.get(i.kind, i.kind), 'version': i.version, 'params_id': i.params_id,
            'log_n': i.log_n, 'nq': i.nq, 'K': i.K, 'body_words': i.body_words}


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f'MI355X engine library missing: {LIB_PATH} (run __graft_entry__.build())')
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        L.fhe_set_coeff_dir(COEFF_DIR.encode())
        _lib = L
    return _lib


def _chk(rc):
    if rc != FHE_OK:
        msg = lib().fhe_last_error().decode()
        if rc == FHE_ENOKEY:
            raise NoKeyError(rc, msg)
        raise FheError(rc, msg)


def _u64(a):
    return a.ctypes.data_as(u64p)


def _dbl(a):
    return a.ctypes.data_as(dp)


def _int(a):
    return a.ctypes.data_as(ip)


class RotationTree:
    """Handle over fhe_rotation_tree_*: build(start, end), rotate(ct, k), stats()."""

    def __init__(self, ctx, N, rots, algo=0):
        r = np.asarray(rots, dtype=np.int32)
        out = C.c_void_p()
        _chk(lib().fhe_rotation_tree_create(ctx.h, N, _int(r), len(r), algo, C.byref(out)))
        self.ctx, self.h = ctx, out.value

    def __del__(self):
        try:
            if self.h:
                lib().fhe_rotation_tree_destroy(self.h)
        except Exception:
            pass

    def build(self, start, end):
        _chk(lib().fhe_rotation_tree_build(self.h, start, end))

    def rotate(self, a, rotation):
        out = C.c_void_p()
        _chk(lib().fhe_rotation_tree_rotate(self.h, a.h, rotation, C.byref(out)))
        return Ct(self.ctx, out.value)

    def stats(self):
        v = (C.c_uint64 * 5)()
        _chk(lib().fhe_rotation_tree_stats(self.h, v))
        return dict(zip(('fast', 'normal', 'total', 'cache_hits', 'cache_misses'), (int(x) for x in v)))


class BootParams(C.Structure):
    """fhe_boot_params (include/fhe_gpu.h)"""
    _fields_ = [('slots', C.c_int), ('level_budget_enc', C.c_int), ('level_budget_dec', C.c_int),
                ('K', C.c_int), ('r', C.c_int), ('degree', C.c_int), ('correction_bits', C.c_int)]


class Bootstrapper:
    """EvalBootstrapSetup(levelBudget, {0, 0}, slots) / EvalBootstrapKeyGen /
    EvalBootstrap on the GPU (fhe_boot_*; tests/k-way/KWaySort235Test.cpp:46-48)."""

    def __init__(self, ctx, slots, budget=(4, 4), K=512, r=6, degree=88, correction_bits=10, keygen=True):
        p = BootParams(slots, budget[0], budget[1], K, r, degree, correction_bits)
        out = C.c_void_p()
        _chk(lib().fhe_boot_create(ctx.h, C.byref(p), C.byref(out)))
        self.ctx, self.h = ctx, out.value
        ctx._boots.append(self)
        if keygen:
            self.keygen()

    def close(self):
        if getattr(self, 'h', None):
            lib().fhe_boot_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def keygen(self):
        _chk(lib().fhe_boot_keygen(self.h))

    @property
    def depth(self):
        return lib().fhe_boot_depth(self.h)

    def rotations(self):
        out = np.zeros(4096, dtype=np.int32)
        m = lib().fhe_boot_rotation_indices(self.h, out.ctypes.data_as(C.POINTER(C.c_int32)), 4096)
        if m < 0:
            _chk(-m)
        return [int(x) for x in out[:m]]

    def bootstrap(self, x, stage=0):
        """fhe_bootstrap_stage: 0 the whole bootstrap, 1..4 its stages; x may be a
        stack (Context.stack) -- member m of the result equals the call on member m"""
        out = C.c_void_p()
        _chk(lib().fhe_bootstrap_stage(self.h, x.h, stage, C.byref(out)))
        return Ct(self.ctx, out.value)

    def mod_raise(self, x): return self.bootstrap(x, 4)
    def coeffs_to_slots(self, x): return self.bootstrap(x, 1)
    def eval_mod(self, x): return self.bootstrap(x, 2)
    def slots_to_coeffs(self, x): return self.bootstrap(x, 3)


class Ct:
    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h

    def __del__(self):
        try:
            if self.h:
                lib().fhe_ct_free(self.h)
        except Exception:
            pass

    def info(self):
        lv, sl, lm, sc = C.c_int(), C.c_int(), C.c_int(), C.c_double()
        _chk(lib().fhe_ct_info(self.h, C.byref(lv), C.byref(sl), C.byref(sc), C.byref(lm)))
        return dict(level=lv.value, slots=sl.value, scale=sc.value, limbs=lm.value)

    @property
    def level(self):
        return self.info()['level']

    @property
    def slots(self):
        return self.info()['slots']

    def set_slots(self, s):
        _chk(lib().fhe_ct_set_slots(self.h, s))

    def data(self):
        inf = self.info()
        out = np.empty((2, inf['limbs'], self.ctx.n), dtype=np.uint64)
        _chk(lib().fhe_ct_download(self.ctx.h, self.h, _u64(out)))
        return out

    def decrypt(self):
        return self.ctx.decrypt(self)


class Pt:
    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h

    def data(self):
        """the plaintext's words [limbs][n] (NTT form)"""
        out = np.empty((lib().fhe_pt_limbs(self.h), self.ctx.n), dtype=np.uint64)
        _chk(lib().fhe_pt_download(self.ctx.h, self.h, _u64(out)))
        return out

    def __del__(self):
        try:
            if self.h:
                lib().fhe_pt_free(self.h)
        except Exception:
            pass


def params_check(logN, L, scale_bits=40, first_bits=60, dnum=3):
    """fhe_params_check: the envelope fhe_ctx_create holds a context to, on the
    host alone.  Returns dict(nq, K, alpha, digits); raises FheError (FHE_EINVAL,
    the parameter named) for a context the kernels cannot serve."""
    p = Params(logN, L, scale_bits, first_bits, dnum, 0)
    v = [C.c_int() for _ in range(4)]
    _chk(lib().fhe_params_check(C.byref(p), *(C.byref(x) for x in v)))
    return dict(zip(('nq', 'K', 'alpha', 'digits'), (x.value for x in v)))


class Context:
    """One engine on one GPU (`device`).  seed 0 (the default): the secret, the
    errors and the encryption randomness come from the OS CSPRNG; a nonzero seed
    makes keys and encryptions reproducible (tests, oracle parity) and must not
    be used to protect data."""

    def __init__(self, logN, L, scale_bits=40, first_bits=60, dnum=3, seed=0, device=0, keygen=True, _handle=None,
                 ps_split=None):
        self.logN, self.n, self.L = logN, 1 << logN, L
        self._boots = []
        self._pair_tables = (0, 0)  # set_pair_tables' current setting
        if _handle is None:
            p = Params(logN, L, scale_bits, first_bits, dnum, seed)
            h = C.c_void_p()
            _chk(lib().fhe_ctx_create(C.byref(p), device, C.byref(h)))
            _handle = h
        self.h = _handle
        nq, K, alpha = C.c_int(), C.c_int(), C.c_int()
        _chk(lib().fhe_ctx_info(self.h, C.byref(nq), C.byref(K), C.byref(alpha), None, None))
        self.nq, self.K, self.alpha = nq.value, K.value, alpha.value
        self.primes = np.empty(self.nq + self.K, dtype=np.uint64)
        self.delta = np.empty(L + 1)
        _chk(lib().fhe_ctx_info(self.h, None, None, None, _u64(self.primes), _dbl(self.delta)))
        if ps_split is not None:
            self.set_ps_split(ps_split)
        if keygen:
            self.keygen()

    # ---- wire format (src/sort.h:31-74, 97-102: Serial::*ToFile, Serialize/DeserializeEval*Key)
    @classmethod
    def deserialize(cls, path, device=0):
        """Serial::DeserializeFromFile(path, cc): a context with no keys."""
        info = wire_inspect(path)
        h = C.c_void_p()
        _chk(lib().fhe_deserialize_context(os.fsencode(path), device, C.byref(h)))
        return cls(int(info['log_n']), int(info['nq']) - 1, keygen=False, _handle=h)

    def serialize(self, path):
        _chk(lib().fhe_serialize_context(self.h, os.fsencode(path)))

    def serialize_public_key(self, path): _chk(lib().fhe_serialize_public_key(self.h, os.fsencode(path)))
    def deserialize_public_key(self, path): _chk(lib().fhe_deserialize_public_key(self.h, os.fsencode(path)))
    def serialize_secret_key(self, path): _chk(lib().fhe_serialize_secret_key(self.h, os.fsencode(path)))
    def deserialize_secret_key(self, path): _chk(lib().fhe_deserialize_secret_key(self.h, os.fsencode(path)))
    def serialize_eval_mult_key(self, path): _chk(lib().fhe_serialize_eval_mult_key(self.h, os.fsencode(path)))
    def deserialize_eval_mult_key(self, path): _chk(lib().fhe_deserialize_eval_mult_key(self.h, os.fsencode(path)))

    def serialize_eval_automorphism_key(self, path):
        _chk(lib().fhe_serialize_eval_automorphism_key(self.h, os.fsencode(path)))

    def deserialize_eval_automorphism_key(self, path):
        n = C.c_int()
        _chk(lib().fhe_deserialize_eval_automorphism_key(self.h, os.fsencode(path), C.byref(n)))
        return n.value

    # seeded switching keys (public stream v1, csrc/wire/wire.hpp): the b halves and
    # the public seed; the deserialize calls above read either format
    def serialize_eval_mult_key_seeded(self, path):
        _chk(lib().fhe_serialize_eval_mult_key_seeded(self.h, os.fsencode(path)))

    def serialize_eval_automorphism_key_seeded(self, path):
        _chk(lib().fhe_serialize_eval_automorphism_key_seeded(self.h, os.fsencode(path)))

    def serialize_ciphertext(self, ct, path):
        _chk(lib().fhe_serialize_ciphertext(self.h, ct.h, os.fsencode(path)))

    def deserialize_ciphertext(self, path):
        h = C.c_void_p()
        _chk(lib().fhe_deserialize_ciphertext(self.h, os.fsencode(path), C.byref(h)))
        return Ct(self, h.value)

    def close(self):
        for b in getattr(self, '_boots', []):  # bootstrappers refer to the context
            b.close()
        if getattr(self, 'h', None):
            lib().fhe_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def digits(self):
        return (self.nq + self.alpha - 1) // self.alpha

    def _new(self, fn, *args):
        out = C.c_void_p()
        _chk(fn(self.h, *args, C.byref(out)))
        return Ct(self, out.value)

    # keys ---------------------------------------------------------------
    def keygen(self):
        _chk(lib().fhe_keygen(self.h))

    def gen_rotation_keys(self, rots):
        r = np.asarray(rots, dtype=np.int32)
        _chk(lib().fhe_gen_rotation_keys(self.h, _int(r), len(r)))

    def load_keys_from(self, orc, rots=()):
        """Upload the CPU oracle's secret/public/relin/rotation keys (parity tests)."""
        s = np.ascontiguousarray(orc.secret_ntt())
        _chk(lib().fhe_ctx_load_secret(self.h, _u64(s)))
        pk = np.ascontiguousarray(orc.public_key())
        _chk(lib().fhe_ctx_load_public(self.h, _u64(pk)))
        rl = np.ascontiguousarray(orc.relin_key())
        keys, idx = [], []
        for k in rots:
            g, key = orc.rot_key(k)
            if g:
                keys.append(np.ascontiguousarray(key))
                idx.append(k)
        arr = (u64p * max(1, len(keys)))(*[_u64(k) for k in keys])
        ia = np.asarray(idx, dtype=np.int32)
        _chk(lib().fhe_ctx_load_keys(self.h, _u64(rl), _int(ia), arr, len(keys)))

    def load_galois_keys_from(self, orc, gs):
        """Upload the oracle's keys of galois elements gs (conjugation: 2n - 1)."""
        for g in gs:
            key = orc.galois_key(g)
            if key is not None:
                _chk(lib().fhe_ctx_load_galois_key(self.h, int(g), _u64(np.ascontiguousarray(key))))

    def gen_galois_keys(self, gs):
        g = np.asarray(gs, dtype=np.uint64)
        _chk(lib().fhe_gen_galois_keys(self.h, _u64(g), len(g)))

    def key_bytes(self):
        return lib().fhe_key_bytes(self.h)

    def set_public_seed(self, seed=None):
        """Keys generated afterwards take their uniform halves from public stream v1
        under `seed` (32 bytes; None: drawn from the OS CSPRNG, refused on a
        context with a test seed)."""
        if seed is not None:
            seed = bytes(seed)
            if len(seed) != 32:
                raise ValueError('a public seed is 32 bytes')
        _chk(lib().fhe_set_public_seed(self.h, seed))

    def get_public_seed(self):
        buf = C.create_string_buffer(32)
        _chk(lib().fhe_get_public_seed(self.h, buf))
        return buf.raw

    def key_is_seeded(self, galois=0):
        """1 / 0 for the key of galois element `galois` (0: the eval-mult key)."""
        r = lib().fhe_key_is_seeded(self.h, int(galois))
        if r < 0:
            _chk(-r)
        return r

    def public_poly(self, seed, kid, digit):
        """a_digit of switching key `kid` under `seed`, [nq + K][n] (kernel parity)."""
        seed = bytes(seed)
        if len(seed) != 32:
            raise ValueError('a public seed is 32 bytes')
        out = np.empty((self.nq + self.K, self.n), dtype=np.uint64)
        _chk(lib().fhe_public_poly(self.h, seed, int(kid), int(digit), _u64(out)))
        return out

    def encode_complex(self, v, slots, level, scale=None):
        v = np.asarray(v, dtype=np.complex128)
        re, im = np.ascontiguousarray(v.real), np.ascontiguousarray(v.imag)
        scale = self.delta[level] if scale is None else scale
        out = C.c_void_p()
        _chk(lib().fhe_pt_encode_complex(self.h, _dbl(re), _dbl(im), len(v), slots, level, scale, C.byref(out)))
        return Pt(self, out.value)

    def conjugate(self, a): return self._new(lib().fhe_conjugate, a.h)

    # objects ------------------------------------------------------------
    def encode(self, v, slots, level=0):
        v = np.ascontiguousarray(v, dtype=np.float64)
        out = C.c_void_p()
        _chk(lib().fhe_pt_encode(self.h, _dbl(v), len(v), slots, level, C.byref(out)))
        return Pt(self, out.value)

    def encode_device(self, v, slots, level=0):
        """fhe_pt_encode_device: encode(v) on the device, word for word"""
        v = np.ascontiguousarray(v, dtype=np.float64)
        out = C.c_void_p()
        _chk(lib().fhe_pt_encode_device(self.h, _dbl(v), len(v), slots, level, C.byref(out)))
        return Pt(self, out.value)

    def encode_masks(self, specs, num_slots, N):
        """fhe_pt_encode_masks: specs = [(kind, k, r, level), ...] -> plaintexts"""
        sp = np.ascontiguousarray(np.asarray(specs, dtype=np.int32).reshape(-1, 4))
        outs = (C.c_void_p * len(sp))()
        _chk(lib().fhe_pt_encode_masks(self.h, sp.ctypes.data_as(C.POINTER(C.c_int32)), len(sp), num_slots, N, outs))
        return [Pt(self, outs[i]) for i in range(len(sp))]

    def set_mask_cache(self, cache):
        """True (default): masks encoded once per context; False: re-encoded on the
        device at the start of every sort (the reference's per-sort encoding)"""
        _chk(lib().fhe_set_mask_cache(self.h, 1 if cache else 0))

    def upload_pt(self, data, level, slots, scale=None):
        data = np.ascontiguousarray(data, dtype=np.uint64)
        scale = self.delta[level] if scale is None else scale
        out = C.c_void_p()
        _chk(lib().fhe_pt_upload(self.h, _u64(data), data.shape[0], level, slots, scale, C.byref(out)))
        return Pt(self, out.value)

    def encrypt(self, v, slots=None, level=0):
        v = np.ascontiguousarray(v, dtype=np.float64)
        return self._new(lib().fhe_encrypt, _dbl(v), len(v), slots or len(v), level)

    def encrypt_ext(self, v, slots=None):
        """FLEXIBLEAUTOEXT-style encryption (lands at level 1, noise / q_L)."""
        v = np.ascontiguousarray(v, dtype=np.float64)
        return self._new(lib().fhe_encrypt_ext, _dbl(v), len(v), slots or len(v))

    def decrypt(self, ct):
        out = np.empty(ct.slots)
        _chk(lib().fhe_decrypt(self.h, ct.h, _dbl(out)))
        return out

    def upload(self, data, level, slots, scale=None):
        data = np.ascontiguousarray(data, dtype=np.uint64)
        scale = self.delta[level] if scale is None else scale
        return self._new(lib().fhe_ct_upload, _u64(data), data.shape[1], level, slots, scale)

    def from_oracle(self, oct):
        inf = oct.info()
        return self.upload(oct.data(), inf['level'], inf['slots'], inf['scale'])

    # ops ----------------------------------------------------------------
    def add(self, a, b): return self._new(lib().fhe_add, a.h, b.h)
    def sub(self, a, b): return self._new(lib().fhe_sub, a.h, b.h)
    def negate(self, a): return self._new(lib().fhe_negate, a.h)
    def add_const(self, a, k): return self._new(lib().fhe_add_const, a.h, k)
    def mul_const(self, a, k): return self._new(lib().fhe_mul_const, a.h, k)
    def mul_const_to(self, a, k, t): return self._new(lib().fhe_mul_const_to, a.h, k, t)
    def mul_int(self, a, k): return self._new(lib().fhe_mul_int, a.h, k)
    def level_adjust(self, a, t): return self._new(lib().fhe_level_adjust, a.h, t)
    def rescale(self, a): return self._new(lib().fhe_rescale, a.h)
    def mul_plain(self, a, p): return self._new(lib().fhe_mul_plain, a.h, p.h)
    def add_plain(self, a, p): return self._new(lib().fhe_add_plain, a.h, p.h)
    def mul(self, a, b): return self._new(lib().fhe_mul_relin, a.h, b.h)
    def square(self, a): return self._new(lib().fhe_square_relin, a.h)

    def mul_add(self, a, b, xs=(), cs=(), raw=None, a_add=None):
        """(a [+ a_add]) * b + sum_i cs[i] xs[i] [+ raw], one relinearisation and one rescale"""
        arr = (C.c_void_p * max(1, len(xs)))(*[x.h for x in xs])
        c = np.ascontiguousarray(cs, dtype=np.float64)
        return self._new(lib().fhe_mul_add, a.h, b.h, arr, _dbl(c), len(xs), None if raw is None else raw.h,
                         None if a_add is None else a_add.h)

    def mul_add_const(self, a, b, xs=(), cs=(), raw=None, a_add=None, a_const=0.0, out_const=0.0):
        """mul_add with (a [+ a_add] + a_const) as the left operand and out_const added to the
        result: the words of add_const before and after the product, formed inside its passes"""
        arr = (C.c_void_p * max(1, len(xs)))(*[x.h for x in xs])
        c = np.ascontiguousarray(cs, dtype=np.float64)
        return self._new(lib().fhe_mul_add_const, a.h, b.h, arr, _dbl(c), len(xs), None if raw is None else raw.h,
                         None if a_add is None else a_add.h, float(a_const), float(out_const))
    def rotate(self, a, k): return self._new(lib().fhe_rotate, a.h, k)

    def rotate_hoisted(self, a, ks):
        ks = np.asarray(ks, dtype=np.int32)
        outs = (C.c_void_p * len(ks))()
        _chk(lib().fhe_rotate_hoisted(self.h, a.h, _int(ks), len(ks), outs))
        return [Ct(self, outs[i]) for i in range(len(ks))]

    def stack(self, xs):
        arr = (C.c_void_p * len(xs))(*[x.h for x in xs])
        out = C.c_void_p()
        _chk(lib().fhe_ct_stack(self.h, arr, len(xs), C.byref(out)))
        return Ct(self, out.value)

    def mul_plain_sum(self, cts, pts):
        ca = (C.c_void_p * len(cts))(*[c.h for c in cts])
        pa = (C.c_void_p * len(pts))(*[p.h for p in pts])
        out = C.c_void_p()
        _chk(lib().fhe_mul_plain_sum(self.h, ca, pa, len(cts), C.byref(out)))
        return Ct(self, out.value)

    def mul_plain_sum_batches(self, cts, pts_per_batch):
        """stack of mul_plain_sum(cts, pts) over the batches' plaintext lists, in one pass"""
        m, nb = len(cts), len(pts_per_batch)
        if any(len(r) != m for r in pts_per_batch):
            raise ValueError('mul_plain_sum_batches: one plaintext per ciphertext in every batch')
        ca = (C.c_void_p * m)(*[c.h for c in cts])
        pa = (C.c_void_p * (m * nb))(*[p.h for r in pts_per_batch for p in r])
        out = C.c_void_p()
        _chk(lib().fhe_mul_plain_sum_batches(self.h, ca, pa, m, nb, C.byref(out)))
        return Ct(self, out.value)

    def member(self, a, m): return self._new(lib().fhe_ct_member, a.h, m)
    def sum_members(self, a): return self._new(lib().fhe_ct_sum_members, a.h)

    def linear_sum_to(self, xs, cs, target):
        arr = (C.c_void_p * len(xs))(*[x.h for x in xs])
        cs = np.ascontiguousarray(cs, dtype=np.float64)
        return self._new(lib().fhe_linear_sum_to, arr, _dbl(cs), len(xs), target)

    def cheb(self, a, coeffs, lo=-1.0, hi=1.0):
        c = np.ascontiguousarray(coeffs, dtype=np.float64)
        return self._new(lib().fhe_cheb_ps, a.h, _dbl(c), len(c), lo, hi)

    def sign(self, a, n, dg, df): return self._new(lib().fhe_sign_composite, a.h, n, dg, df)
    def compare(self, a, b, n, dg, df): return self._new(lib().fhe_compare, a.h, b.h, n, dg, df)
    def indicator(self, a, c, n, dg, df): return self._new(lib().fhe_indicator, a.h, c, n, dg, df)

    def rotation_tree(self, N, rots, algo=0):
        """RotationTree<N>(cc, rots, algo) (src/rotation.h:240-358); algo 0 = NAF."""
        return RotationTree(self, N, rots, algo)

    def compose_rotate(self, a, N, rots, algo, rotation):
        r = np.asarray(rots, dtype=np.int32)
        return self._new(lib().fhe_compose_rotate, a.h, N, _int(r), len(r), algo, rotation)

    def compose_rotate_members(self, a, N, rots, algo, rotations):
        """member m of the batch `a` rotated by rotations[m], steps batched across members"""
        r = np.asarray(rots, dtype=np.int32)
        k = np.asarray(rotations, dtype=np.int32)
        return self._new(lib().fhe_compose_rotate_members, a.h, N, _int(r), len(r), algo, _int(k), len(k))

    def direct_sort(self, x, N, rots, cfg, mode=0, rank=None, shard=(0, 1), allreduce=None):
        r = np.asarray(rots, dtype=np.int32)
        hk = _Hook(allreduce)
        try:
            return self._new(lib().fhe_direct_sort, x.h, rank.h if rank is not None else None, N, _int(r), len(r),
                             cfg[0], cfg[1], cfg[2], mode, shard[0], shard[1], hk.ptr(), None)
        except FheError as e:
            hk.reraise(e)

    def direct_sort_columns(self, key, cols, N, rots, cfg, rank=None, shard=(0, 1), allreduce=None):
        """Records sorted by an encrypted key (fhe_direct_sort_columns): out[p] is
        rotationIndexCheckN(rank(key), cols[p]) -- what direct_sort(cols[p], mode=2,
        rank=...) gives, word for word -- with the index series evaluated once for
        all columns.  rank=None: the rank is constructed from `key`; with a rank,
        key may be None.  Pass the key among cols to get it sorted too.  With tied
        keys the columns mix exactly as the key does (tests/tie_model.py) unless
        set_sort_tiebreak is set: then they come out in the stable permutation."""
        r = np.asarray(rots, dtype=np.int32)
        cols = list(cols)
        arr = (C.c_void_p * max(1, len(cols)))(*[None if c is None else c.h for c in cols])
        outs = (C.c_void_p * max(1, len(cols)))()
        hk = _Hook(allreduce)
        try:
            _chk(lib().fhe_direct_sort_columns(self.h, None if key is None else key.h,
                                               None if rank is None else rank.h, arr, len(cols), N, _int(r), len(r),
                                               cfg[0], cfg[1], cfg[2], shard[0], shard[1], hk.ptr(), None, outs))
        except FheError as e:
            hk.reraise(e)
        return [Ct(self, outs[i]) for i in range(len(cols))]

    def direct_select(self, key, targets, N, rots, cfg, cols=None, rank=None):
        """Order statistics by encrypted rank (fhe_direct_select): out[c] has N
        slots, slot p < len(targets) holds cols[c]'s value at the element whose rank
        is targets[p] (ranks 0..N-1, any order, repeats allowed), the other slots
        hold zero.  cols=None: the key is the one column and its select is returned
        (not a list).  rank=None: the rank is constructed from `key`; with a rank
        (direct_sort mode 1), key may be None when cols are given.  Up to P_ - 1
        targets (num_slots = N * P_) cost one index series on one ciphertext.  With
        tied keys the result mixes values exactly as the sort does
        (tests/tie_model.py) unless set_sort_tiebreak is set: then the order
        statistics are exact."""
        r = np.asarray(rots, dtype=np.int32)
        t = np.ascontiguousarray(targets, dtype=np.int32).reshape(-1)
        single = cols is None
        cols = [key] if single else list(cols)
        arr = (C.c_void_p * max(1, len(cols)))(*[None if c is None else c.h for c in cols])
        outs = (C.c_void_p * max(1, len(cols)))()
        _chk(lib().fhe_direct_select(self.h, None if key is None else key.h, None if rank is None else rank.h, arr,
                                     len(cols), t.ctypes.data_as(C.POINTER(C.c_int32)), len(t), N, _int(r), len(r),
                                     cfg[0], cfg[1], cfg[2], outs))
        res = [Ct(self, outs[i]) for i in range(len(cols))]
        return res[0] if single else res

    def encode_select(self, targets, member, num_slots, N, level_c, level_k):
        """fhe_pt_encode_select: (C, K) of one member of a select, encoded on the device"""
        t = np.ascontiguousarray(targets, dtype=np.int32).reshape(-1)
        outs = (C.c_void_p * 2)()
        _chk(lib().fhe_pt_encode_select(self.h, t.ctypes.data_as(C.POINTER(C.c_int32)), len(t), member, num_slots, N,
                                        level_c, level_k, outs))
        return Pt(self, outs[0]), Pt(self, outs[1])

    def mul_plain_sum_groups(self, stack, pts, groups):
        """member g = mul_plain_sum(members g * len(pts) .. of the stack, pts), all groups in one pass"""
        pa = (C.c_void_p * max(1, len(pts)))(*[p.h for p in pts])
        return self._new(lib().fhe_mul_plain_sum_groups, stack.h, pa, len(pts), groups)

    @staticmethod
    def select_layout(N, num_slots, ntargets):
        return select_layout(N, num_slots, ntargets)

    def set_sort_tiebreak(self, eps):
        """Tie-breaking for keys with equal values (fhe_set_sort_tiebreak): with
        0 < eps < 0.5 every rank built afterwards (direct_sort modes 0 and 1,
        direct_sort_columns / direct_select without a rank, sort_hybrid) is the
        stable argsort rank -- earlier index first among equals -- at the plain
        sort's depth and output level.  Distinct values must differ by >= 2 eps,
        the sign configuration must resolve eps, and |x_i - x_j| + eps <= 1.
        0 (the default) is the reference's rank."""
        _chk(lib().fhe_set_sort_tiebreak(self.h, float(eps)))

    def set_pair_tables(self, n_left, n_right):
        """Tables of different sizes (fhe_set_pair_tables): group_sum, running_sum,
        window_sum and gather called afterwards pair a left table of n_left rows
        (its keys, bounds and positions in n_left slots) with a right table of
        n_right rows (its keys, positions and every column in n_right slots), N =
        max(n_left, n_right), and return outputs of n_left slots, at
        pair_shape(...)'s batch count.  (0, 0), the default, is the square call."""
        _chk(lib().fhe_set_pair_tables(self.h, int(n_left), int(n_right)))
        self._pair_tables = (int(n_left), int(n_right))

    @staticmethod
    def pair_shape(n_left, n_right, ring_slots):
        return pair_shape(n_left, n_right, ring_slots)

    @contextlib.contextmanager
    def _tables(self, tables):
        """the pair tables of one call: set for its duration, the previous setting restored after it"""
        if tables is None:
            yield
            return
        prev = self._pair_tables
        self.set_pair_tables(*tables)
        try:
            yield
        finally:
            self.set_pair_tables(*prev)

    def encode_tiebreak(self, batches, num_slots, N, eps, level):
        """fhe_pt_encode_tiebreak: the offsets of the given comparator batches,
        filled and encoded on the device as one batch"""
        b = np.ascontiguousarray(batches, dtype=np.int32).reshape(-1)
        outs = (C.c_void_p * max(1, len(b)))()
        _chk(lib().fhe_pt_encode_tiebreak(self.h, b.ctypes.data_as(C.POINTER(C.c_int32)), len(b), num_slots, N,
                                          float(eps), level, outs))
        return [Pt(self, outs[i]) for i in range(len(b))]

    def sub_add_plain_stacked(self, a, bs, ps):
        """stack whose member i is add_plain(sub(a, bs[i]), ps[i]) word for word, in one pass"""
        ba = (C.c_void_p * max(1, len(bs)))(*[b.h for b in bs])
        pa = (C.c_void_p * max(1, len(ps)))(*[p.h for p in ps])
        if len(bs) != len(ps):
            raise ValueError('sub_add_plain_stacked: one plaintext per operand')
        return self._new(lib().fhe_sub_add_plain_stacked, a.h, ba, pa, len(bs))

    def group_sum(self, left_key, right_key, cols, eps, N, rots, cfg, count=False, tables=None):
        """Group sums and lookups (fhe_direct_group_sum): out[p] has N slots, slot e
        holds the sum of cols[p] over the right rows j with |left_key_e - right_key_j|
        < eps.  right_key = left_key: SUM(v) OVER (PARTITION BY key), the row itself
        included; another table's key and columns: the LEFT JOIN lookup, zero where
        no right key matches.  count=True: returns (outs, count), the count holding
        the number of matching right rows.  Equal keys must agree far below eps,
        distinct keys differ by >= 2 eps, |difference| + eps <= 1, and the sign
        configuration must resolve eps; 0 < eps < 0.5.  A column may sit at
        group_sum_levels(...)[0] at most; the outputs end at the rank's level.
        tables=(Nl, Nr): set_pair_tables for this call -- left_key in Nl slots, right_key
        and cols in Nr, N = max(Nl, Nr), outputs of Nl slots."""
        r = np.asarray(rots, dtype=np.int32)
        cols = list(cols)
        arr = (C.c_void_p * max(1, len(cols)))(*[None if c is None else c.h for c in cols])
        outs = (C.c_void_p * max(1, len(cols)))()
        cnt = C.c_void_p()
        with self._tables(tables):
            _chk(lib().fhe_direct_group_sum(self.h, None if left_key is None else left_key.h,
                                            None if right_key is None else right_key.h, arr, len(cols), float(eps), N,
                                            _int(r), len(r), cfg[0], cfg[1], cfg[2], outs,
                                            C.byref(cnt) if count else None))
        res = [Ct(self, outs[i]) for i in range(len(cols))]
        return (res, Ct(self, cnt.value)) if count else res

    @staticmethod
    def group_sum_levels(key_level, cfg):
        return group_sum_levels(key_level, cfg)

    def sub_pm_const_stacked(self, a, bs, c):
        """stack of 2 len(bs) members: member i is add_const(sub(a, bs[i]), c), member
        len(bs) + i is add_const(negate(sub(a, bs[i])), c), word for word, in one pass"""
        ba = (C.c_void_p * max(1, len(bs)))(*[b.h for b in bs])
        return self._new(lib().fhe_sub_pm_const_stacked, a.h, ba, len(bs), float(c))

    def mul_pairs(self, a, a_add, b_stack, ncols):
        """the B-member stacks a, a_add against the column-major stack b_stack of
        ncols * B members: member p * B + z of the result is
        mul(add(member(a, z), member(a_add, z)), member(b_stack, p * B + z)) word for word"""
        return self._new(lib().fhe_mul_pairs, a.h, a_add.h, b_stack.h, ncols)

    def gather(self, pos_l, pos_r, cols, offsets, N, rots, present=False, sum_offsets=False, tables=None):
        """Gather by encrypted position (fhe_direct_gather): for column p and offset k
        the output has N slots, slot e holds cols[p] at the right row j whose position
        pos_r[j] equals pos_l[e] + offsets[k], zero where there is none.  The positions
        hold integers in [0, N) up to a rank's noise, the right ones distinct; |offset|
        <= N - 1.  Returns the gathered columns column-major (index p * K + k);
        present=True returns (outs, flags), flags[k] holding 1 where the neighbour
        exists.  sum_offsets=True adds the offsets' indicators before the product: one
        output per column, the sum over the offsets (ROWS BETWEEN), and one flag, the
        frame's row count.  A column may sit at gather_levels(...)[0] at most.
        tables=(Nl, Nr): set_pair_tables for this call -- pos_l in Nl slots, pos_r and
        cols in Nr, N = max(Nl, Nr), outputs of Nl slots."""
        r = np.asarray(rots, dtype=np.int32)
        off = np.asarray(list(offsets), dtype=np.int32)
        cols = list(cols)
        ko = 1 if sum_offsets else len(off)
        nout = (len(cols) + (1 if present else 0)) * ko
        arr = (C.c_void_p * max(1, len(cols)))(*[None if c is None else c.h for c in cols])
        outs = (C.c_void_p * max(1, nout))()
        with self._tables(tables):
            _chk(lib().fhe_direct_gather(self.h, None if pos_l is None else pos_l.h,
                                         None if pos_r is None else pos_r.h, arr, len(cols), _int(off), len(off),
                                         int(bool(present)), int(bool(sum_offsets)), N, _int(r), len(r), outs))
        res = [Ct(self, outs[i]) for i in range(nout)]
        return (res[:len(cols) * ko], res[len(cols) * ko:]) if present else res

    def lag(self, rank, cols, k, N, rots, present=False):
        """LAG(v, k) in rank order: gather with pos_l = pos_r = rank and offset -k"""
        return self.gather(rank, rank, cols, [-int(k)], N, rots, present=present)

    def lead(self, rank, cols, k, N, rots, present=False):
        """LEAD(v, k) in rank order: gather with pos_l = pos_r = rank and offset +k"""
        return self.gather(rank, rank, cols, [int(k)], N, rots, present=present)

    @staticmethod
    def gather_levels(pos_level, N):
        return gather_levels(pos_level, N)

    def sub_offsets_stacked(self, a, bs, offsets):
        """stack of len(offsets) * len(bs) members: member k * len(bs) + i is
        add_const(sub(a, bs[i]), offsets[k]), negated for offsets[k] < 0, word for word,
        in one pass"""
        ba = (C.c_void_p * max(1, len(bs)))(*[b.h for b in bs])
        off = np.asarray(list(offsets), dtype=np.int32)
        return self._new(lib().fhe_sub_offsets_stacked, a.h, ba, len(bs), _int(off), len(off))

    def mul_gather(self, a_stack, b_stack, ncols, noffsets):
        """the noffsets * B-member stack a_stack (member k * B + z) against the
        column-major stack b_stack of ncols * B members: member (p * noffsets + k) * B + z
        of the result is mul(member(a_stack, k * B + z), member(b_stack, p * B + z)) word
        for word"""
        return self._new(lib().fhe_mul_gather, a_stack.h, b_stack.h, ncols, noffsets)

    def running_sum(self, left_key, right_key, cols, eps, N, rots, cfg, mode=RUN_ROWS, lo=None, count=False,
                    tables=None):
        """Running sums (fhe_direct_running_sum): out[p] has N slots, slot e holds the
        sum of cols[p] over the right rows j that the mode selects for left row e:
        RUN_ROWS the rows up to and including e in the stable key order (right_key =
        left_key: SUM(v) OVER (ORDER BY key ROWS UNBOUNDED PRECEDING)), RUN_LE
        right_key_j <= left_key_e (the default RANGE frame, the range lookup,
        searchsorted side='right' with the count), RUN_LT right_key_j < left_key_e
        (side='left'), RUN_BETWEEN lo_e <= right_key_j <= left_key_e with left_key the
        upper bound and lo required (the band join, the sliding RANGE window).
        count=True: returns (outs, count), the count holding the number of selected
        right rows; with RUN_ROWS and right_key = left_key, count - 1 is the stable
        rank.  Equal keys must agree far below eps, distinct keys and bounds differ
        by >= 2 eps, every difference +- eps lie in [-1, 1], and the sign
        configuration must resolve eps; 0 < eps < 0.5.  Levels are group_sum_levels'.
        tables=(Nl, Nr): set_pair_tables for this call -- left_key and lo in Nl slots,
        right_key and cols in Nr, N = max(Nl, Nr), outputs of Nl slots; RUN_ROWS is
        refused between unequal sizes."""
        r = np.asarray(rots, dtype=np.int32)
        cols = list(cols)
        arr = (C.c_void_p * max(1, len(cols)))(*[None if c is None else c.h for c in cols])
        outs = (C.c_void_p * max(1, len(cols)))()
        cnt = C.c_void_p()
        with self._tables(tables):
            _chk(lib().fhe_direct_running_sum(self.h, None if left_key is None else left_key.h,
                                              None if lo is None else lo.h,
                                              None if right_key is None else right_key.h, arr, len(cols), int(mode),
                                              float(eps), N, _int(r), len(r), cfg[0], cfg[1], cfg[2], outs,
                                              C.byref(cnt) if count else None))
        res = [Ct(self, outs[i]) for i in range(len(cols))]
        return (res, Ct(self, cnt.value)) if count else res

    def sub_bounds_stacked(self, as_, bs, consts):
        """stack of len(as_) len(bs) members (1 or 2 left operands): member v len(bs) + i
        is add_const(sub(as_[v], bs[i]), consts[v]) word for word, in one pass"""
        if len(as_) != len(consts):
            raise ValueError('sub_bounds_stacked: one constant per left operand')
        aa = (C.c_void_p * max(1, len(as_)))(*[a.h for a in as_])
        ba = (C.c_void_p * max(1, len(bs)))(*[b.h for b in bs])
        cs = np.ascontiguousarray(consts, dtype=np.float64).reshape(-1)
        return self._new(lib().fhe_sub_bounds_stacked, aa, len(as_), ba, len(bs), _dbl(cs))

    def mul_pairs_const(self, a, c, b_stack, ncols):
        """the B-member stack a against the column-major stack b_stack of ncols * B
        members: member p * B + z of the result is
        mul(add_const(member(a, z), c), member(b_stack, p * B + z)) word for word"""
        return self._new(lib().fhe_mul_pairs_const, a.h, float(c), b_stack.h, ncols)

    def mul_pairs_sub(self, a, a_sub, b_stack, ncols):
        """as mul_pairs_const with the left operand sub(member(a, z), member(a_sub, z))"""
        return self._new(lib().fhe_mul_pairs_sub, a.h, a_sub.h, b_stack.h, ncols)

    def lex_rank(self, keys, eps, N, rots, cfg):
        """Lexicographic rank (fhe_direct_lex_rank): slot e holds the position of row
        e among the N rows ordered by keys[0], then keys[1], ... (2 to 4 single
        ciphertexts at one level, most significant first) -- ORDER BY a, b, or one
        wide key split into digits.  With set_sort_tiebreak set it is the stable
        lexicographic argsort rank; without it rows tied on every key share their
        ranks as the plain rank's ties do.  Values equal on a leading key must agree
        far below eps, distinct ones differ by >= 2 eps, |difference| + eps <= 1, and
        the sign configuration must resolve eps; 0 < eps < 0.5.  The rank ends at
        lex_rank_levels(...) and feeds direct_sort(mode=2), direct_sort_columns and
        direct_select as any rank does."""
        r = np.asarray(rots, dtype=np.int32)
        keys = list(keys)
        arr = (C.c_void_p * max(1, len(keys)))(*[None if k is None else k.h for k in keys])
        out = C.c_void_p()
        _chk(lib().fhe_direct_lex_rank(self.h, arr, len(keys), float(eps), N, _int(r), len(r), cfg[0], cfg[1], cfg[2],
                                       C.byref(out)))
        return Ct(self, out.value)

    def lex_sort_columns(self, keys, cols, eps, N, rots, cfg):
        """Records ordered by several encrypted keys: lex_rank(keys), then
        direct_sort_columns(rank=...) of cols.  Pass keys among cols to get them
        sorted too.  The context needs the sort's depth plus len(keys) - 1."""
        return self.direct_sort_columns(None, cols, N, rots, cfg, rank=self.lex_rank(keys, eps, N, rots, cfg))

    @staticmethod
    def lex_rank_levels(key_level, nkeys, cfg):
        return lex_rank_levels(key_level, nkeys, cfg)

    def sub_lex_stacked(self, as_, bs, eps, ps=None):
        """fhe_sub_lex_stacked: with L = len(as_) keys and bs key-major (L * count
        ciphertexts), the stack of (2 L - 1) * count members: for a leading key l,
        member 2 l count + i is add_const(sub(as_[l], bs[l count + i]), eps) and member
        (2 l + 1) count + i the same with -eps; for the last key, member
        2 (L - 1) count + i is sub(as_[L - 1], bs[...]) [add_plain ps[i]]; word for word"""
        L = len(as_)
        if L == 0 or len(bs) % L:
            raise ValueError('sub_lex_stacked: one operand list per key')
        count = len(bs) // L
        if ps is not None and len(ps) != count:
            raise ValueError('sub_lex_stacked: one plaintext per operand')
        aa = (C.c_void_p * max(1, L))(*[a.h for a in as_])
        ba = (C.c_void_p * max(1, len(bs)))(*[b.h for b in bs])
        pa = None if ps is None else (C.c_void_p * max(1, count))(*[p.h for p in ps])
        return self._new(lib().fhe_sub_lex_stacked, aa, L, ba, count, pa, float(eps))

    def mul_lex(self, t, t_const, u, w):
        """member z = mul(add_const(member(t, z), t_const), sub(member(u, z), member(w, z)))
        word for word, in one tensor pass where t, u and w share a level"""
        return self._new(lib().fhe_mul_lex, t.h, float(t_const), u.h, w.h)

    def window_sum(self, part_left, part_right, cols, eps, N, rots, cfg, order_left=None, order_right=None,
                   mode=WIN_GROUP, lo=None, count=False, tables=None):
        """Window sums (fhe_direct_window_sum): out[p] has N slots, slot e holds the sum
        of cols[p] over the right rows j that agree with left row e on every partition
        key (part_left[g]_e = part_right[g]_j, 1 to 3 keys; the same handles for a self
        join) and that the order key selects: WIN_ROWS / WIN_LE / WIN_LT / WIN_BETWEEN
        are running_sum's modes on (order_left, order_right, lo) inside the partition
        -- SUM(v) OVER (PARTITION BY g ORDER BY t ...), the as-of join, the
        per-partition sliding window -- and WIN_GROUP (no order key; at least two
        partition keys) is GROUP BY a, b and the join on several keys.  count=True:
        returns (outs, count), the number of selected right rows (ROW_NUMBER() under
        WIN_ROWS).  running_sum's conditions hold for every key; levels are
        window_sum_levels(key_level, len(part_left) + (mode != WIN_GROUP), cfg).
        tables=(Nl, Nr): set_pair_tables for this call -- part_left, order_left and lo in
        Nl slots, part_right, order_right and cols in Nr, N = max(Nl, Nr), outputs of Nl
        slots; WIN_ROWS is refused between unequal sizes."""
        r = np.asarray(rots, dtype=np.int32)
        cols, part_left, part_right = list(cols), list(part_left), list(part_right)
        if len(part_left) != len(part_right):
            raise ValueError('window_sum: one right partition key per left one')
        h = lambda x: None if x is None else x.h
        pl = (C.c_void_p * max(1, len(part_left)))(*[h(k) for k in part_left])
        pr = (C.c_void_p * max(1, len(part_right)))(*[h(k) for k in part_right])
        arr = (C.c_void_p * max(1, len(cols)))(*[h(c) for c in cols])
        outs = (C.c_void_p * max(1, len(cols)))()
        cnt = C.c_void_p()
        with self._tables(tables):
            _chk(lib().fhe_direct_window_sum(self.h, pl, pr, len(part_left), h(order_left), h(lo), h(order_right),
                                             arr, len(cols), int(mode), float(eps), N, _int(r), len(r), cfg[0],
                                             cfg[1], cfg[2], outs, C.byref(cnt) if count else None))
        res = [Ct(self, outs[i]) for i in range(len(cols))]
        return (res, Ct(self, cnt.value)) if count else res

    @staticmethod
    def window_sum_levels(key_level, nfactors, cfg):
        return window_sum_levels(key_level, nfactors, cfg)

    def sub_window_stacked(self, part_as, part_bs, eps, mode=WIN_GROUP, order_a=None, order_bs=None, order_lo=None,
                           ps=None):
        """fhe_sub_window_stacked: with G = len(part_as) partition keys and part_bs
        key-major (G * count ciphertexts), members (2 g) count + i and (2 g + 1) count + i
        are add_const(sub(part_as[g], part_bs[g count + i]), +eps / -eps); from member
        2 G count on the order key's by mode: WIN_ROWS add_plain(sub(order_a,
        order_bs[i]), ps[i]), WIN_LE / WIN_LT add_const(sub(order_a, order_bs[i]), +eps /
        -eps), WIN_BETWEEN that with +eps, then add_const(sub(order_lo, order_bs[i]),
        -eps); WIN_GROUP none; word for word"""
        G = len(part_as)
        if G == 0 or len(part_bs) % G:
            raise ValueError('sub_window_stacked: one operand list per partition key')
        count = len(part_bs) // G
        if order_bs is not None and len(order_bs) != count:
            raise ValueError('sub_window_stacked: one order operand per partition operand')
        if ps is not None and len(ps) != count:
            raise ValueError('sub_window_stacked: one plaintext per operand')
        arr = lambda xs: None if xs is None else (C.c_void_p * max(1, len(xs)))(*[x.h for x in xs])
        return self._new(lib().fhe_sub_window_stacked, arr(part_as), G, arr(part_bs), count, int(mode),
                         None if order_a is None else order_a.h, None if order_lo is None else order_lo.h,
                         arr(order_bs), arr(ps), float(eps))

    def mul_sub_sub(self, u, w, u2, w2):
        """member z = mul(sub(member(u, z), member(w, z)), sub(member(u2, z), member(w2, z)))
        word for word, in one tensor pass where the four share a level"""
        return self._new(lib().fhe_mul_sub_sub, u.h, w.h, u2.h, w2.h)

    def mul_columns(self, a, cols):
        """the stack a (B members) times each single ciphertext of cols: member
        p * B + z of the result is mul(member(a, z), cols[p]) word for word"""
        arr = (C.c_void_p * max(1, len(cols)))(*[c.h for c in cols])
        return self._new(lib().fhe_mul_columns, a.h, arr, len(cols))

    def sum_member_groups(self, a, groups):
        """stack of `groups` members: member p = the sum of a's members p * B .. p * B + B - 1"""
        return self._new(lib().fhe_ct_sum_member_groups, a.h, groups)

    def set_sort_column_members(self, m):
        """most members (columns x stacked batches) of one stacked column product
        of direct_sort_columns; the words do not depend on it"""
        _chk(lib().fhe_set_sort_column_members(self.h, m))

    def sort_hybrid(self, x, N, rots, cfg, mode=0, rank=None, max_array=256, mask=0, shard=(0, 1), allreduce=None):
        """DirectSort::sort_hybrid (mode 0) or rotationIndexCheckHybrid(rank, x) (mode 1)."""
        r = np.asarray(rots, dtype=np.int32)
        hk = _Hook(allreduce)
        try:
            return self._new(lib().fhe_sort_hybrid, x.h, rank.h if rank is not None else None, N, _int(r), len(r),
                             cfg[0], cfg[1], cfg[2], mode, max_array, mask, shard[0], shard[1], hk.ptr(), None)
        except FheError as e:
            hk.reraise(e)

    def mehp24_sort(self, x, N, cfg, dg_i, df_i, sub=0, shard=(0, 1), allreduce=None):
        """mehp24::sortFG (sub 0; x holds N values in N*N slots) or
        sortLargeArrayFG with parts of `sub` values (x in sub*sub slots).
        shard=(rank, world): the pair compares and indicators are split over
        ranks and combined by `allreduce` (or RCCL after comm_init)."""
        if shard == (0, 1) and allreduce is None:
            return self._new(lib().fhe_mehp24_sort, x.h, N, sub, cfg[0], cfg[1], cfg[2], dg_i, df_i)
        hk = _Hook(allreduce)
        try:
            return self._new(lib().fhe_mehp24_sort_sharded, x.h, N, sub, cfg[0], cfg[1], cfg[2], dg_i, df_i,
                             shard[0], shard[1], hk.ptr(), None)
        except FheError as e:
            hk.reraise(e)

    def mehp24_indicator(self, x, b, dg, df):
        return self._new(lib().fhe_mehp24_indicator, x.h, b, dg, df)

    def kway_sort(self, x, k, M, cfg, boot=None):
        """kwaySort::Sorter::sorter via KWayAdapter<k^M>::sort; cfg = (3, dg, df).
        boot: a Bootstrapper (checkLevelAndBoot + compositeSign's lazy bootstrap);
        the number of checkLevelAndBoot bootstraps is left in self.kway_bootstraps."""
        if boot is None:
            return self._new(lib().fhe_kway_sort, x.h, k, M, cfg[1], cfg[2])
        nb = C.c_int()
        out = self._new(lib().fhe_kway_sort_boot, x.h, k, M, cfg[1], cfg[2], boot.h, C.byref(nb))
        self.kway_bootstraps = nb.value
        return out

    def check_level_and_boot(self, x, need, boot=None):
        """EvalUtils::checkLevelAndBoot: (ciphertext, booted)."""
        b = C.c_int()
        out = self._new(lib().fhe_check_level_and_boot, x.h, need, boot.h if boot is not None else None, C.byref(b))
        return out, bool(b.value)

    def kway_sorter(self, kk, xs, cmps):
        """SortUtils::fcnL (kk = 1) or the kk-sorter (kk = 2..5): ascending outputs."""
        xa = (C.c_void_p * len(xs))(*[x.h for x in xs])
        ca = (C.c_void_p * len(cmps))(*[c.h for c in cmps])
        nout = 1 if kk == 1 else kk
        outs = (C.c_void_p * nout)()
        _chk(lib().fhe_kway_sorter(self.h, kk, xa, len(xs), ca, len(cmps), outs))
        return [Ct(self, outs[i]) for i in range(nout)]

    # multi-GPU -----------------------------------------------------------
    @staticmethod
    def comm_unique_id():
        buf = (C.c_uint8 * 128)()
        _chk(lib().fhe_comm_get_unique_id(buf))
        return bytes(buf)

    def comm_init(self, uid, rank, world):
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        _chk(lib().fhe_comm_init(self.h, buf, rank, world))

    def pool_trim(self):
        _chk(lib().fhe_pool_trim(self.h))

    def pool_stats(self):
        v = [C.c_uint64() for _ in range(3)]
        _chk(lib().fhe_pool_stats(self.h, *[C.byref(x) for x in v]))
        return {'live': v[0].value, 'cached': v[1].value, 'peak': v[2].value}

    def set_sort_lanes(self, m):
        _chk(lib().fhe_set_sort_lanes(self.h, m))

    def set_kway_stack(self, on):
        """k = 5 stages run their two compares (and the pair's bootstraps) as one
        2-member stack (fhe_set_kway_stack); the words do not depend on it"""
        _chk(lib().fhe_set_kway_stack(self.h, 1 if on else 0))

    def set_ps_split(self, split):
        """PS_SPLIT_OPENFHE (default) or PS_SPLIT_ENGINE (fhe_set_ps_split)"""
        _chk(lib().fhe_set_ps_split(self.h, int(split)))

    @property
    def ps_split(self):
        return int(lib().fhe_get_ps_split(self.h))

    def set_sort_stack(self, m):
        _chk(lib().fhe_set_sort_stack(self.h, m))

    def ct_allreduce(self, ct):
        _chk(lib().fhe_ct_allreduce(self.h, ct.h))

    # kernel level -------------------------------------------------------
    def ntt(self, prime_index, data, inverse=False):
        d = np.ascontiguousarray(data, dtype=np.uint64).copy()
        limbs = 1 if d.ndim == 1 else d.shape[0]
        _chk(lib().fhe_ntt(self.h, _u64(d), prime_index, limbs, 1 if inverse else 0))
        return d

    def ntt_dev(self, dev_ptr, first_prime, limbs, inverse=False, segments=1, seg_stride=0, stream=None):
        """fhe_ntt_dev: in place on device memory, enqueued on `stream` (hipStream_t
        as an int, None = the context stream); returns without synchronising"""
        _chk(lib().fhe_ntt_dev(self.h, C.c_void_p(dev_ptr), first_prime, limbs, segments, seg_stride,
                               1 if inverse else 0, C.c_void_p(stream) if stream else None))

    def automorph_dev(self, dev_in, limbs, galois, dev_out, stream=None):
        _chk(lib().fhe_automorph_dev(self.h, C.c_void_p(dev_in), limbs, galois, C.c_void_p(dev_out),
                                     C.c_void_p(stream) if stream else None))

    def modup(self, d):
        d = np.ascontiguousarray(d, dtype=np.uint64)
        ell = d.shape[0]
        digits = (ell + self.alpha - 1) // self.alpha
        out = np.empty((digits, ell + self.K, self.n), dtype=np.uint64)
        _chk(lib().fhe_modup(self.h, _u64(d), ell, _u64(out)))
        return out

    def moddown(self, x):
        x = np.ascontiguousarray(x, dtype=np.uint64)
        ell = x.shape[0] - self.K
        out = np.empty((ell, self.n), dtype=np.uint64)
        _chk(lib().fhe_moddown(self.h, _u64(x), ell, _u64(out)))
        return out

    def linear_sums_raw(self, xs, K, sh, level, consts=None):
        """the multi-output sums of products behind linear_sums_to's doubles: K, sh
        [G][m] integers (the constant K 2^sh, |K| <= 2^62), consts = (Kc, shc) of [G]
        or None; G unrescaled sums at `level` (fhe_linear_sums_raw)"""
        K = np.ascontiguousarray(K, dtype=np.int64)
        sh = np.ascontiguousarray(sh, dtype=np.uint8)
        G, m = K.shape
        if sh.shape != K.shape or m != len(xs):
            raise ValueError('linear_sums_raw: K and sh are [G][len(xs)]')
        i64p, u8p = C.POINTER(C.c_int64), C.POINTER(C.c_uint8)
        kc = sc = None
        if consts is not None:
            kc = np.ascontiguousarray(consts[0], dtype=np.int64)
            sc = np.ascontiguousarray(consts[1], dtype=np.uint8)
            if kc.shape != (G,) or sc.shape != (G,):
                raise ValueError('linear_sums_raw: one folded constant per output')
        arr = (C.c_void_p * m)(*[x.h for x in xs])
        outs = (C.c_void_p * G)()
        _chk(lib().fhe_linear_sums_raw(self.h, arr, m, K.ctypes.data_as(i64p), sh.ctypes.data_as(u8p), G,
                                       None if kc is None else kc.ctypes.data_as(i64p),
                                       None if sc is None else sc.ctypes.data_as(u8p), level, outs))
        return [Ct(self, outs[g]) for g in range(G)]

    def automorph(self, x, g):
        x = np.ascontiguousarray(x, dtype=np.uint64)
        out = np.empty_like(x)
        _chk(lib().fhe_automorph(self.h, _u64(x), x.shape[0], g, _u64(out)))
        return out

    def counters(self):
        out = np.zeros(7, dtype=np.uint64)
        _chk(lib().fhe_counters(self.h, _u64(out)))
        return dict(zip(['hmult', 'keyswitch', 'rotations', 'rescale', 'ptmult', 'constmult', 'opbytes'],
                        map(int, out)))

    def collective_stats(self):
        """{'allreduce_s': host seconds inside the sharded sorts' partial-sum
        exchanges since reset_counters(), 'allreduce_calls': their count}"""
        out = np.zeros(2, dtype=np.uint64)
        _chk(lib().fhe_collective_stats(self.h, _u64(out)))
        return {'allreduce_s': int(out[0]) * 1e-9, 'allreduce_calls': int(out[1])}

    def boot_counters(self):
        """{'calls': bootstrap passes since reset_counters(), 'ciphertexts': the
        ciphertexts they refreshed (a stack of B: one pass, B ciphertexts)}"""
        out = np.zeros(2, dtype=np.uint64)
        _chk(lib().fhe_boot_counters(self.h, _u64(out)))
        return {'calls': int(out[0]), 'ciphertexts': int(out[1])}

    def region_marker(self, begin):
        """k_region_begin / k_region_end on the context stream (profiling)"""
        _chk(lib().fhe_region_marker(self.h, 1 if begin else 0))

    def reset_counters(self):
        _chk(lib().fhe_reset_counters(self.h))

    def sync(self):
        _chk(lib().fhe_sync(self.h))

    def stream(self):
        return lib().fhe_stream(self.h)


def time_kernel(ctx, name, limbs, iters=20):
    ms, b = C.c_double(), C.c_double()
    _chk(lib().fhe_time_kernel(ctx.h, name.encode(), limbs, iters, C.byref(ms), C.byref(b)))
    return {'name': name, 'avg_ms': ms.value, 'bytes': b.value}


class KernelClock:
    """Live per-launch clock over real work (HIP events on the engine stream
    around every NTT pass): `with KernelClock(ctx) as k: ...; k.stats`."""

    def __init__(self, ctx):
        self.ctx, self.stats = ctx, None

    def __enter__(self):
        _chk(lib().fhe_kernel_clock_start(self.ctx.h))
        return self

    def __exit__(self, *exc):
        import json
        need = C.c_size_t()
        buf = C.create_string_buffer(1 << 20)
        _chk(lib().fhe_kernel_clock_stop(self.ctx.h, buf, len(buf), C.byref(need)))
        if need.value > len(buf):
            raise FheError(FHE_EINTERNAL, 'kernel clock report truncated')
        self.stats = json.loads(buf.value.decode())
        return False


def host_stats(reset=False):
    """process-wide host costs (fhe_host_stats): encodes, encode s, pool-miss mallocs, malloc s"""
    out = np.zeros(4)
    _chk(lib().fhe_host_stats(_dbl(out)))
    if reset:
        _chk(lib().fhe_host_stats_reset())
    return {'encodes': int(out[0]), 'encode_s': round(float(out[1]), 4), 'mallocs': int(out[2]),
            'malloc_s': round(float(out[3]), 4)}


def prng_block(key, counter, nonce):
    """ChaCha20 block of the secure sampler (fhe_prng_block), 16 u32 words"""
    k = np.ascontiguousarray(key, dtype=np.uint32)
    nn = np.ascontiguousarray(nonce, dtype=np.uint32)
    out = np.zeros(16, dtype=np.uint32)
    P32 = C.POINTER(C.c_uint32)
    _chk(lib().fhe_prng_block(k.ctypes.data_as(P32), int(counter), nn.ctypes.data_as(P32), out.ctypes.data_as(P32)))
    return out


def cheb_ps_uses_openfhe(coeffs):
    """True iff the OpenFHE split evaluates these coefficients with its division
    tree (fhe_cheb_ps_plan; False: the power-of-two fallback)"""
    c = np.ascontiguousarray(coeffs, dtype=np.float64)
    r = lib().fhe_cheb_ps_plan(c.ctypes.data_as(C.POINTER(C.c_double)), len(c))
    if r < 0:
        raise FheError(-r, lib().fhe_last_error().decode())
    return r == 1


def cheb_ps_depth(degree, split=PS_SPLIT_OPENFHE):
    """levels a degree-d Chebyshev series consumes under `split` (fhe_cheb_ps_depth)"""
    r = lib().fhe_cheb_ps_depth(int(degree), int(split))
    if r < 0:
        raise FheError(-r, lib().fhe_last_error().decode())
    return r


def size_parameters(N):
    d = C.c_int()
    rots = np.zeros(512, dtype=np.int32)
    m = lib().fhe_size_parameters(N, C.byref(d), _int(rots), 512)
    if m < 0:
        raise FheError(-m, lib().fhe_last_error().decode())
    return d.value, [int(x) for x in rots[:m]]


def group_sum_levels(key_level, cfg):
    """fhe_group_sum_levels (pure host): (col_max_level, out_level) of group_sum for
    keys at key_level under the composite sign cfg = (n, dg, df)"""
    col, out = C.c_int(), C.c_int()
    rc = lib().fhe_group_sum_levels(int(key_level), cfg[0], cfg[1], cfg[2], C.byref(col), C.byref(out))
    if rc != FHE_OK:
        raise FheError(rc, lib().fhe_last_error().decode())
    return col.value, out.value


def gather_levels(pos_level, N):
    """fhe_gather_levels (pure host): (col_max_level, series_level, out_level) of gather
    for positions at pos_level over N rows; the present flags end at series_level"""
    col, ser, out = C.c_int(), C.c_int(), C.c_int()
    rc = lib().fhe_gather_levels(int(pos_level), int(N), C.byref(col), C.byref(ser), C.byref(out))
    if rc != FHE_OK:
        raise FheError(rc, lib().fhe_last_error().decode())
    return col.value, ser.value, out.value


def window_sum_levels(key_level, nfactors, cfg):
    """fhe_window_sum_levels (pure host): (col_max_level, out_level) of window_sum for
    keys at key_level and nfactors factors (the partition keys, plus one for an
    order key) under the composite sign cfg = (n, dg, df)"""
    col, out = C.c_int(), C.c_int()
    rc = lib().fhe_window_sum_levels(int(key_level), int(nfactors), cfg[0], cfg[1], cfg[2], C.byref(col), C.byref(out))
    if rc != FHE_OK:
        raise FheError(rc, lib().fhe_last_error().decode())
    return col.value, out.value


def lex_rank_levels(key_level, nkeys, cfg):
    """fhe_lex_rank_levels (pure host): the level lex_rank's result ends at for nkeys
    keys at key_level under the composite sign cfg = (n, dg, df)"""
    out = C.c_int()
    rc = lib().fhe_lex_rank_levels(int(key_level), int(nkeys), cfg[0], cfg[1], cfg[2], C.byref(out))
    if rc != FHE_OK:
        raise FheError(rc, lib().fhe_last_error().decode())
    return out.value


def select_layout(N, num_slots, ntargets):
    """fhe_select_layout (pure host): (members, member[p], start[p]) of a select of
    ntargets targets over num_slots = N * P_ slots.  cap = P_ - 1 (1 when P_ = 1)
    targets share a member; target p owns the cyclic window of N slots from
    start[p] (= p mod N) on."""
    k = max(1, int(ntargets))
    member, start = np.zeros(k, dtype=np.int32), np.zeros(k, dtype=np.int32)
    i32 = C.POINTER(C.c_int32)
    m = lib().fhe_select_layout(N, num_slots, ntargets, member.ctypes.data_as(i32), start.ctypes.data_as(i32), k)
    if m < 0:
        raise FheError(-m, lib().fhe_last_error().decode())
    return m, [int(x) for x in member], [int(x) for x in start]


def pair_shape(n_left, n_right, ring_slots):
    """fhe_pair_shape (pure host): (num_slots, num_partition, num_batch, np, fold_steps)
    of an all-pairs call between tables of n_left and n_right rows on a ring of
    ring_slots = n / 2 slots; the first four in stable_model.rank_shape's order"""
    v = [C.c_int() for _ in range(5)]
    rc = lib().fhe_pair_shape(int(n_left), int(n_right), int(ring_slots), *[C.byref(x) for x in v])
    if rc != FHE_OK:
        raise FheError(rc, lib().fhe_last_error().decode())
    P, nb, S, npb, fold = (x.value for x in v)
    return S, P, nb, npb, fold


def tiebreak_offsets(N, num_slots, batch, eps):
    """fhe_tiebreak_offsets (pure host): the +-eps offsets of comparator batch
    `batch` of a rank over num_slots slots"""
    out = np.empty(max(int(num_slots), 0), dtype=np.float64)
    _chk(lib().fhe_tiebreak_offsets(N, num_slots, batch, float(eps), _dbl(out)))
    return out


def mehp24_parameters(N):
    """The reference MEHP24 test's parameters for N (Mehp24SortTest.cpp:26-128)."""
    v = [C.c_int() for _ in range(7)]
    cfg = np.zeros(3, dtype=np.int32)
    rots = np.zeros(1024, dtype=np.int32)
    m = lib().fhe_mehp24_parameters(N, *(C.byref(x) for x in v[:4]), _int(cfg), *(C.byref(x) for x in v[4:]),
                                    _int(rots), 1024)
    if m < 0:
        raise FheError(-m, lib().fhe_last_error().decode())
    depth, log_ring, scale, dnum, dg_i, df_i, sub = (x.value for x in v)
    return dict(depth=depth, log_ring=log_ring, scale_bits=scale, dnum=dnum, cfg=tuple(int(c) for c in cfg), dg_i=dg_i,
                df_i=df_i, sub=sub, rots=[int(x) for x in rots[:m]])


def hybrid_parameters(N):
    """The hybrid sort test's (depth, rotations) for N (tests/DirectSortHTest.cpp:23-104)."""
    d = C.c_int()
    rots = np.zeros(256, dtype=np.int32)
    m = lib().fhe_hybrid_parameters(N, C.byref(d), _int(rots), 256)
    if m < 0:
        raise FheError(-m, lib().fhe_last_error().decode())
    return d.value, [int(x) for x in rots[:m]]


def mehp24_rotation_indices(N, sub=256):
    rots = np.zeros(1024, dtype=np.int32)
    m = lib().fhe_mehp24_rotation_indices(N, sub, _int(rots), 1024)
    if m < 0:
        raise FheError(-m, lib().fhe_last_error().decode())
    return [int(x) for x in rots[:m]]


def kway_rotation_indices(N):
    rots = np.zeros(64, dtype=np.int32)
    m = lib().fhe_kway_rotation_indices(N, _int(rots), 64)
    if m < 0:
        raise FheError(-m, lib().fhe_last_error().decode())
    return [int(x) for x in rots[:m]]


def kway_stage_count(k, M):
    return int(lib().fhe_kway_stage_count(k, M))


def kway_sort_type(k, M, stage):
    v = [C.c_int() for _ in range(3)]
    _chk(lib().fhe_kway_sort_type(k, M, stage, *[C.byref(a) for a in v]))
    return tuple(a.value for a in v)


def kway_rotate_distance(k, log_dist, slope):
    return int(lib().fhe_kway_rotate_distance(k, log_dist, slope))


def kway_gen_indices(num_slots, k, M, m, log_dist, slope):
    g = np.zeros(num_slots, dtype=np.int32)
    p = np.zeros(num_slots, dtype=np.int32)
    _chk(lib().fhe_kway_gen_indices(num_slots, k, M, m, log_dist, slope, _int(g), _int(p)))
    return g, p


def decompose(N, rots, rotation, wrapN, algo):
    r = np.asarray(rots, dtype=np.int32)
    vals = np.zeros(128, dtype=np.int32)
    sizes = np.zeros(128, dtype=np.int32)
    m = lib().fhe_decompose(N, _int(r), len(r), rotation, wrapN, algo, _int(vals), _int(sizes), 128)
    if m < 0:
        raise FheError(-m, lib().fhe_last_error().decode())
    return [(int(vals[i]), int(sizes[i])) for i in range(m)]
