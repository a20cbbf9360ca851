// The parameter envelope: what the kernels' dispatch tables and argument
// structs can serve.  host::envelope_params (hostmath.cpp) refuses a context
// outside it before any HIP call; the launch sites that own a table hold their
// table to these numbers with static_asserts, so the two cannot drift apart.
#pragma once

namespace fhe_envelope {
// ring: the wire format's range (wire.cpp read_context).  Below it the
// point-wise kernels' n / NT grids and blocks of 256 or 512 coefficients
// (k_modup_fp, k_modup_fold, k_expand_uniform's 1 << (logN - 3)) stop holding;
// above it ntt.hip dispatch() has no column pass (PB = ceil(logN / 2) <= 9).
constexpr int LOG_N_MIN = 10, LOG_N_MAX = 17;
// digits at the top level: ModUpArgs holds 8 per-digit pointers and bounds
// (kernels.hip), and ks_inner, ks_inner_mc, k_ntt_row_ks and the hoisted
// rotations dispatch dispatch_int<1, 8>(digits)
constexpr int MAX_DIGITS = 8;
// digit width alpha: dispatch_int<1, 24>(at) of k_modup_convert / k_modup_fp
// (the folded ModUp takes at <= 32 and k_modup_mfma 24, so 24 serves every form)
constexpr int MAX_DIGIT_WIDTH = 24;
// special primes K: dispatch_int<1, 16>(K) of every ModDown kernel
constexpr int MAX_SPECIAL = 16;
}  // namespace fhe_envelope
