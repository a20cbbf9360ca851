// MI355X RNS-CKKS ciphertext-op engine — host-side C++ interface.
//
// One Engine per GPU (one process per GPU).  Ciphertexts live in HBM for
// their whole life: [2][limbs][n] u64 in NTT (evaluation) form.  Every op is
// enqueued on the engine's HIP stream; nothing synchronises the host except
// downloads/decryption.  The op set and its semantics (levels, canonical
// scales, rounding of constants) are the spec of DESIGN.md §3, which the CPU
// oracle (oracle/) restates independently; results are bit-identical.
//
// The reference reaches these operations through OpenFHE's CryptoContext
// (EvalAdd/EvalSub/EvalMult/EvalSquare/EvalMultAndRelinearize/EvalRotate/
// EvalFastRotation/EvalChebyshevSeriesPS, called from src/sign.cpp,
// src/comparison.cpp, src/rotation.h and src/sort_algo.h).
#pragma once
#include <array>
#include <complex>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../host/hostmath.hpp"

namespace fhe {

using u64 = uint64_t;
using i64 = int64_t;
using PublicSeed = std::array<uint8_t, 32>;  // public stream v1 (csrc/wire/wire.hpp)

struct DevMem;  // pooled device allocation (engine.hip)

// An A/B switch from the environment: the integer value of `name`, `dflt` when
// it is unset.  Every call site keeps the result in a function-local static, so
// a switch is read once per process.
inline int env_switch(const char *name, int dflt) {
    const char *e = std::getenv(name);
    return e ? std::atoi(e) : dflt;
}

// A ciphertext batch: `batch` independent ciphertexts at one level, stored
// [batch][2][limbs][n].  Every op applies member-wise in the same launches, so
// the comparator / index-check pipelines of all rank-sort batches run as one
// (DESIGN.md §6).  batch = 1 is an ordinary ciphertext.
struct Ciphertext {
    std::shared_ptr<DevMem> mem;
    u64 *data = nullptr;  // [batch][2][limbs][n]
    int level = 0;
    int slots = 0;
    double scale = 0;
    size_t limbs = 0;
    int batch = 1;
};
using CtPtr = std::shared_ptr<Ciphertext>;

struct Plaintext {
    std::shared_ptr<DevMem> mem;
    u64 *data = nullptr;  // [limbs][n]
    int level = 0;
    int slots = 0;
    double scale = 0;
    size_t limbs = 0;
};
using PtPtr = std::shared_ptr<Plaintext>;

struct Counters {
    u64 hmult = 0, keyswitch = 0, rotations = 0, rescale = 0, ptmult = 0, constmult = 0;
    // op-level algorithmic HBM bytes (SURVEY §8(d)'s per-op formulas, each op
    // at its own level; B = 8n per limb): HMult (4l + 2 digits(l)(l+K) + 2l) B,
    // rotation (2l + 2 digits(l)(l+K) + 2l) B, ct x pt 5l B, ct x const 4l B,
    // add 6l B, linear sum of m terms (2l m + 2l) B -- per ciphertext
    u64 opbytes = 0;
    // sharded runs: host wall time inside the partial-sum exchanges (header +
    // data all-reduce, from a drained stream to the reduced data), and their count
    u64 allreduce_ns = 0, allreduce_calls = 0;
    // Bootstrapper::evalBootstrap calls and the ciphertexts they refreshed (a
    // stack of B counts once and B times)
    u64 boot_calls = 0, boot_cts = 0;
    Counters &operator+=(const Counters &o) {
        boot_calls += o.boot_calls;
        boot_cts += o.boot_cts;
        opbytes += o.opbytes;
        allreduce_ns += o.allreduce_ns;
        allreduce_calls += o.allreduce_calls;
        hmult += o.hmult;
        keyswitch += o.keyswitch;
        rotations += o.rotations;
        rescale += o.rescale;
        ptmult += o.ptmult;
        constmult += o.constmult;
        return *this;
    }
};

// Paterson-Stockmeyer split used by evalChebyshevSeriesPS (csrc/algo): OpenFHE's
// (k, m) long-division split (the default, as the reference), or the
// power-of-two split of rounds 1-2
enum : int { PS_SPLIT_ENGINE = 0, PS_SPLIT_OPENFHE = 1 };

class Engine {
  public:
    Engine(int logN, int L, int scale_bits, int first_bits, int dnum, int device, u64 seed);
    // the Paterson-Stockmeyer split, one value shared by this engine and every
    // fork of it (lane engines cached by the sorters read the current split, so
    // a change after a sort cannot leave lanes on the old one)
    int ps_split() const { return *ps_split_; }
    void set_ps_split(int split) { *ps_split_ = split; }
    ~Engine();
    // A second engine on its own HIP stream and memory pool sharing this one's
    // keys and tables: independent work issued to both (from two host threads)
    // runs concurrently on the GPU.  Keys must be complete before forking.
    std::unique_ptr<Engine> fork() const;
    // order this engine's stream after everything enqueued on `other` so far
    void wait_for(const Engine &other);
    Engine(const Engine &) = delete;
    Engine &operator=(const Engine &) = delete;

    const host::Params &params() const;
    size_t n() const;
    double delta(int level) const;

    // ------------------------------------------------------------ keys ---
    void keygen();
    void gen_rotation_keys(const std::vector<int> &rot);
    void load_secret(const u64 *s_ntt);           // [nall][n]
    void load_public(const u64 *pk);              // [2][nq][n]
    void load_relin(const u64 *key);              // [digits][2][nall][n]
    void load_rotation(long k, const u64 *key);   // [digits][2][nall][n]
    bool has_rotation_key(long k) const;
    // keys of arbitrary automorphisms X -> X^g (rotations: g = 5^k; conjugation: 2n - 1)
    void gen_galois_keys(const std::vector<u64> &gs);
    void load_galois(u64 g, const u64 *key);      // [digits][2][nall][n]
    bool has_galois_key(u64 g) const;
    size_t key_bytes() const;
    // key export (wire format, csrc/wire): same layouts as the loads above;
    // a missing key throws std::invalid_argument
    int key_digits() const;
    size_t switch_key_words() const;              // digits * 2 * nall * n
    bool has_secret() const;
    bool has_public() const;
    bool has_relin() const;
    void export_secret(u64 *out);
    void export_public(u64 *out);
    void export_relin(u64 *out);
    std::vector<u64> galois_elements() const;     // ascending
    void export_galois(u64 g, u64 *out);
    // Seeded switching keys (public stream v1, csrc/wire/wire.hpp).  With a public
    // seed set, the keys generated afterwards take their uniform halves a_j from
    // the seed's stream, expanded on the device, and are recorded as seeded; a
    // key loaded in full is not.  key_seeded: 1 (seed, if given, receives the
    // key's seed) / 0 / -1 no such key; kid 0 = relinearisation key, else the
    // galois element.
    void set_public_seed(const uint8_t seed[32]);
    bool get_public_seed(uint8_t seed[32]) const;
    int key_seeded(u64 kid, uint8_t *seed = nullptr) const;
    // a_digit of key `kid` under `seed` over all nq + K primes, [nall][n] to host
    void public_poly(const uint8_t seed[32], u64 kid, int digit, u64 *out);
    // the b halves alone, [digits][nall][n]; the loads expand the a halves
    void export_relin_b(u64 *out);
    void export_galois_b(u64 g, u64 *out);
    void load_relin_seeded(const uint8_t seed[32], const u64 *b);
    void load_galois_seeded(const uint8_t seed[32], u64 g, const u64 *b);

    // ------------------------------------------------- encode / encrypt ---
    PtPtr encode(const std::vector<double> &v, int slots, int level);
    PtPtr encode_scaled(const std::vector<double> &v, int slots, int level, double scale);
    PtPtr encode_complex(const std::vector<std::complex<double>> &v, int slots, int level, double scale);
    // the same plaintext over Q_level u P (ell + K limbs, special primes last)
    PtPtr encode_complex_ext(const std::vector<std::complex<double>> &v, int slots, int level, double scale);
    // Device encoding (csrc/device/encode.hip), word-identical to encode():
    // the special inverse FFT, rounding, RNS split and NTT of a batch in a few
    // launches.  encode_masks generates the sort's public masks on the device
    // (kind 0: mask_vector(k) rotated by r, kind 1: checking_vector(k),
    // src/sort_algo.h:206-233, 272-286; slots num_slots, block size N);
    // encode_device takes arbitrary real slot vectors.
    struct MaskSpec {
        int kind, k, r, level;
    };
    std::vector<PtPtr> encode_masks(const std::vector<MaskSpec> &specs, int num_slots, int N);
    std::vector<PtPtr> encode_device(const std::vector<std::vector<double>> &vs, int slots, const std::vector<int> &levels);
    // The two plaintexts of member `member` of an order-statistic select
    // (DirectSortN::selectColumns; layout: select_layout): {C at level_c, K at
    // level_k}.  C holds targets[p] on the window of every target p of the member,
    // K holds 1 at each window's first slot, both 0 elsewhere.  The slot vectors
    // are filled on the device (k_select_slots) from the member's targets; each
    // plaintext equals encode() of its vector word for word.
    std::array<PtPtr, 2> encode_select(const std::vector<int> &targets, int member, int num_slots, int N, int level_c,
                                       int level_k);
    // Tie-break offsets of the rank's comparator batches (DirectSortN::constructRank,
    // DESIGN.md §6.3).  Slot s of batch b compares element e = s mod N with element
    // (e + t) mod N, t = b num_slots / N + s / N; the offset is +eps where that
    // element is e itself or precedes it (t == 0 or e + t >= N), -eps elsewhere.
    // tiebreak_offsets is the host definition; encode_tiebreak fills the vectors
    // of a list of batches on the device (k_tiebreak_slots) and encodes them as
    // one batch at `level`, each plaintext equal to encode() of its vector word
    // for word.
    static std::vector<double> tiebreak_offsets(int N, int num_slots, int batch, double eps);
    std::vector<PtPtr> encode_tiebreak(const std::vector<int> &batches, int num_slots, int N, double eps, int level);
    // targets per member (cap) of that layout; throws unless N and num_slots / N
    // are powers of two with num_slots / N <= N
    static int select_cap(int N, int num_slots);
    CtPtr encrypt(const std::vector<double> &v, int slots, int level = 0);
    CtPtr encrypt_pt(const Plaintext &pt);
    // OpenFHE FLEXIBLEAUTOEXT-style encryption: one extra level absorbs the
    // encryption noise (divided by q_L); the result sits at level 1
    CtPtr encrypt_ext(const std::vector<double> &v, int slots);
    std::vector<double> decrypt(const Ciphertext &ct);
    CtPtr upload(const u64 *host, size_t limbs, int level, int slots, double scale);
    void download(const Ciphertext &ct, u64 *host);
    PtPtr upload_pt(const u64 *host, size_t limbs, int level, int slots, double scale);

    // -------------------------------------------------------------- ops ---
    CtPtr clone(const Ciphertext &a);
    CtPtr add(const Ciphertext &a, const Ciphertext &b);
    CtPtr sub(const Ciphertext &a, const Ciphertext &b);
    void add_inplace(CtPtr &acc, const Ciphertext &b);
    CtPtr negate(const Ciphertext &a);
    CtPtr add_plain(const Ciphertext &a, const Plaintext &p);
    CtPtr sub_plain(const Ciphertext &a, const Plaintext &p);
    CtPtr plain_sub(const Plaintext &p, const Ciphertext &a);
    CtPtr add_const(const Ciphertext &a, double c);
    // a = a + c, in place on the c0 limbs when a is exclusively owned (else add_const)
    void add_const_inplace(CtPtr &a, double c);
    CtPtr mul_int(const Ciphertext &a, i64 k);
    CtPtr mul_const(const Ciphertext &a, double c);
    CtPtr mul_const_to(const Ciphertext &a, double c, int target);
    CtPtr level_adjust(const Ciphertext &a, int target);
    void match_levels(CtPtr &a, CtPtr &b);
    void count_bytes(double limb_units, int members);
    double ks_units(size_t ell) const;
    CtPtr mul_plain(const Ciphertext &a, const Plaintext &p);
    // sum_i a_i * p_i with one rescale (masked sums of src/sort_algo.h:341-346, 573-577)
    CtPtr mul_plain_sum(const std::vector<const Ciphertext *> &a, const std::vector<const Plaintext *> &p);
    CtPtr mul(const Ciphertext &a, const Ciphertext &b);
    // a*b + sum_i c_i x_i with one rescale (lazy rescaling of PS remainders)
    // a_add (optional): the left operand is a + a_add, formed inside the tensor
    // pass (same words as add(a, a_add) first)
    // a_const (0 = none): a constant at a's scale added to the left operand after
    // a_add, on load in the tensor pass (the words of add_const(add(a, a_add), c));
    // out_const (0 = none): a constant at the result's scale, added to d0 in the
    // tensor pass times the prime the rescale drops (the HMult tail is linear in
    // d0 and divides by that prime: the words of add_const on the product).  FHE_MUL_FOLD_CONST=0 or
    // an operand that is level-adjusted first takes the separate launches.
    CtPtr mul_add(const Ciphertext &a, const Ciphertext &b, const std::vector<const Ciphertext *> &xs,
                  const std::vector<double> &cs, const Ciphertext *raw = nullptr, const Ciphertext *a_add = nullptr,
                  double a_const = 0.0, double out_const = 0.0);
    // whether mul_add forms a + a_const on load: only where add_const would see
    // the operand the tensor loads, i.e. a is not level-adjusted against b
    static bool mul_fold_left(bool enabled, int a_level, int b_level) { return enabled && a_level >= b_level; }
    // the masked sums of nb batches over one list of ciphertexts in one pass:
    // member b of the result is mul_plain_sum(a, p[b]) word for word (one kernel
    // over all batches, one rescale of the 2 nb segments).  Every a_i is a single
    // ciphertext; FHE_RANK_STACK_MASKS=0 runs the nb sums and stacks them.
    CtPtr mul_plain_sum_batches(const std::vector<const Ciphertext *> &a,
                                const std::vector<std::vector<const Plaintext *>> &p);
    // the masked sums of `groups` groups of Z = p.size() consecutive members of
    // the stack a against one plaintext list: member g of the result is
    // mul_plain_sum({member(a, g Z + z)}_z, p) word for word (one kernel,
    // k_mul_plain_sum_groups, over all groups, one rescale of the 2 `groups`
    // segments).  FHE_SELECT_FUSED=0 (A/B): one mul_plain_sum per group, stacked.
    CtPtr mul_plain_sum_groups(const Ciphertext &a, const std::vector<const Plaintext *> &p, int groups);
    // same with the sum already formed: raw = linear_sums_to(xs, {c}, level+1, false)[0]
    CtPtr mul_add_raw(const Ciphertext &a, const Ciphertext &b, const Ciphertext &raw, const Ciphertext *a_add = nullptr,
                      double a_const = 0.0, double out_const = 0.0);
    // the stack a (B members) times each of P single ciphertexts: member p B + z
    // of the result is mul(member(a, z), *cols[p]) word for word.  One tensor pass
    // (k_tensor_cols), then mul's relinearisation / rescale tail on P B members.
    // A column at a level lower than a's is level-adjusted to it as mul would; one
    // at a higher level is refused (mul would adjust a instead, and the products
    // would not share a level).  FHE_SORT_COLS_FUSED=0
    // (A/B): P broadcast mul calls, stacked.
    CtPtr mul_columns(const Ciphertext &a, const std::vector<const Ciphertext *> &cols);
    // the B-member stacks a and a_add against the column-major stack b of P B
    // members, all at one level: member p B + z of the result is
    // mul(add(member(a, z), member(a_add, z)), member(b, p B + z)) word for word.
    // One tensor pass (k_tensor_pairs: a + a_add formed once per thread for up to
    // four columns), then mul's relinearisation / rescale tail on P B members.
    // FHE_GROUP_FUSED=0 (A/B): P mul_add(a, column p of b, a_add) calls, stacked.
    CtPtr mul_pairs(const Ciphertext &a, const Ciphertext &a_add, const Ciphertext &b, int P);
    CtPtr square(const Ciphertext &a);
    CtPtr rotate(const Ciphertext &a, long k);
    std::vector<CtPtr> rotate_hoisted(const Ciphertext &a, const std::vector<long> &ks);
    // member m of a batch rotated by ks[m] (all keyed): the giant steps of a
    // BSGS linear transform as one pipeline
    CtPtr rotate_members(const Ciphertext &a, const std::vector<long> &ks);
    // x + sum_k rotate(x, k) with one ModUp and one ModDown (the key products of
    // every rotation summed over Q u P, the rotated c0s added after the ModDown;
    // oracle: Context::rotate_sum_hoisted) -- the bootstrap's partial trace
    CtPtr rotate_sum_hoisted(const Ciphertext &x, const std::vector<long> &ks);
    // Double-hoisted baby-step giant-step linear transform (oracle:
    // Context::linear_transform_ext): one ModUp of x, the baby rotations kept
    // over Q u P and multiplied there by extended plaintexts (encode_complex_ext),
    // the unrotated giant as the starting accumulator, every rotated giant brought
    // down, rotated and summed over Q u P, one final ModDown, then the rescale.
    // Both take stacks: every member goes through the same launches (one ModUp
    // of all members, the member-blocked key kernels of kernels.hpp, the rotated
    // giants of all members as one key-switch input set); one ciphertext keeps
    // the single-ciphertext launches.
    struct LtGiant {
        long shift = 0;
        std::vector<int> baby;               // indices into `baby`
        std::vector<const Plaintext *> pts;  // extended plaintexts at x's level
    };
    CtPtr linear_transform_ext(const Ciphertext &x, const std::vector<long> &baby, const std::vector<LtGiant> &giants);
    // keyed automorphisms sharing one ModUp; conjugate = g 2n - 1
    std::vector<CtPtr> apply_galois_hoisted(const Ciphertext &a, const std::vector<u64> &gs);
    CtPtr conjugate(const Ciphertext &a);
    // ModRaise (bootstrapping): last-level ciphertext (one limb) re-read over
    // every Q prime by the centred lift; level 0, scale Delta_0
    CtPtr mod_raise(const Ciphertext &a);
    CtPtr rescale(const Ciphertext &a);
    CtPtr drop_to(const Ciphertext &a, int level);
    CtPtr linear_sum_to(const std::vector<const Ciphertext *> &xs, const std::vector<double> &c, int target);
    // several linear sums of the same inputs (PS leaves): one output per row of c
    // (rescale = false: the raw sums at level target-1 and the pre-rescale scale, for mul_add_raw)
    // consts (rescaled sums only): one constant per output, added as add_const would
    // add it, inside the sum kernel (no pass of its own)
    std::vector<CtPtr> linear_sums_to(const std::vector<const Ciphertext *> &xs,
                                      const std::vector<std::vector<double>> &c, int target, bool rescale = true,
                                      const std::vector<double> *consts = nullptr);
    // linear_sums_to behind its doubles (a device-level test hook): the constants
    // as the pairs (K, sh) the kernels take, K [G][m] with |K| <= 2^62 standing for
    // K 2^sh, Kc / shc [G] or null the folded constants.  G unrescaled sums at
    // `level` through the same tables, launches and passes as linear_sums_to
    // (with Kc: + Kc 2^shc q_last on c0 below the last limb)
    std::vector<CtPtr> linear_sums_raw(const std::vector<const Ciphertext *> &xs, const int64_t *K, const uint8_t *sh,
                                       size_t G, const int64_t *Kc, const uint8_t *shc, int level);
    CtPtr trivial_const(double c, int level, int slots, int batch = 1);
    CtPtr zero_like(int level, int slots, int batch = 1);
    // batches: stack (copies; equal levels), member view (no copy), member sum
    CtPtr stack(const std::vector<const Ciphertext *> &xs);
    CtPtr member(const Ciphertext &a, int m);
    // batches built in place (no stack copies): member i = a - bs[i] (a brought to
    // the bs' level once), and member i = a - ps[i]
    CtPtr sub_stacked(const Ciphertext &a, const std::vector<const Ciphertext *> &bs);
    CtPtr sub_plain_stacked(const Ciphertext &a, const std::vector<const Plaintext *> &ps);
    // member i = add_plain(sub(a, bs[i]), ps[i]) word for word, written straight
    // into the stack by one launch (k_sub_add_plain_stacked: a's words loaded once
    // per tile of members).  sub_stacked's level rules: a at a lower level than
    // the bs is level-adjusted once, a at a higher one takes per-member ops; the
    // ps sit at the differences' level.  FHE_TIEBREAK_FUSED=0 (A/B): sub_stacked,
    // then c0 += ps[i] per member.
    CtPtr sub_add_plain_stacked(const Ciphertext &a, const std::vector<const Ciphertext *> &bs,
                                const std::vector<const Plaintext *> &ps);
    // with B = bs.size(): member i = add_const(sub(a, bs[i]), c) and member B + i =
    // add_const(negate(sub(a, bs[i])), c) word for word, written straight into the
    // 2 B stack by one launch (k_sub_pm_const_stacked: each bs[i] loaded once for
    // both members, a's words once per tile of members).  The constant enters c0
    // with add_const's residues at the differences' scale.  sub_stacked's level
    // rules.  FHE_GROUP_FUSED=0 (A/B): sub_stacked, then negate / add_const on
    // the stack, stacked.
    CtPtr sub_pm_const_stacked(const Ciphertext &a, const std::vector<const Ciphertext *> &bs, double c);
    // The oriented, offset differences of the gather (DirectSortN::gatherColumns,
    // DESIGN.md §6.8): with B = bs.size() and K = offsets.size(), member k B + i =
    // add_const(sub(a, bs[i]), offsets[k]) for an offset >= 0 and the negate of that
    // for an offset < 0, word for word, written straight into the K B stack by one
    // launch (k_sub_offsets_stacked: each bs[i] loaded once for all offsets, a's
    // words once per tile of members).  sub_stacked's level rules.
    // FHE_GATHER_FUSED=0 (A/B): sub_stacked, then add_const / negate on the stack
    // per offset, stacked.
    CtPtr sub_offsets_stacked(const Ciphertext &a, const std::vector<const Ciphertext *> &bs,
                              const std::vector<int> &offsets);
    // the K B-member stack a (member k B + z) against the column-major stack b of
    // P B members, all at one level: member (p K + k) B + z of the result is
    // mul(member(a, k B + z), member(b, p B + z)) word for word.  One tensor pass
    // (k_tensor_gather: a column's words loaded once per thread for up to four
    // offsets), then mul's relinearisation / rescale tail on P K B members.
    // FHE_GATHER_FUSED=0 (A/B): one stacked mul per (column, offset), stacked.
    CtPtr mul_gather(const Ciphertext &a, const Ciphertext &b, int P, int K);
    // The differences of lexicographic keys (DirectSortN::lexRank):
    // with L = as.size() keys (2..4), count = bs.size() / L and bs key-major
    // (bs[l count + i]), the result is a stack of (2 L - 1) count members: for a
    // leading key l < L - 1, member (2 l) count + i = add_const(sub(*as[l], b), eps)
    // and member (2 l + 1) count + i = add_const(sub(*as[l], b), -eps); for the last
    // key, member 2 (L - 1) count + i = sub(*as[L - 1], b), with add_plain(., *ps[i])
    // when ps is not empty; word for word, written by one launch
    // (k_sub_lex_stacked: each b loaded once, a key's words once per tile).  The
    // as share a level and so do the bs; sub_stacked's level rules: as at a lower
    // level are level-adjusted once, at a higher one every member takes its own
    // ops; the ps sit at the differences' level.  FHE_LEX_FUSED=0 (A/B):
    // sub_stacked and add_const per key, stacked.
    CtPtr sub_lex_stacked(const std::vector<const Ciphertext *> &as, const std::vector<const Ciphertext *> &bs,
                          const std::vector<const Plaintext *> &ps, double eps);
    // member z = mul(add_const(member(t, z), t_const), sub(member(u, z), member(w, z)))
    // word for word for the B-member stacks t, u, w (u and w at one level).  With t
    // at that level too, one tensor pass (k_tensor_lex) adds the constant to c0 as
    // it loads t and forms u - w as it loads them, then mul's relinearisation /
    // rescale tail; with t at another level (mul would level-adjust an operand) or
    // under FHE_LEX_FUSED=0 it is sub, then the product.
    CtPtr mul_lex(const Ciphertext &t, double t_const, const Ciphertext &u, const Ciphertext &w);
    // The bounded differences of the running sums (DirectSortN::runningSums,
    // DESIGN.md §6.6): with V = as.size() left operands (1 or 2, single ciphertexts
    // at one level), one constant each and B = bs.size(), member v B + i =
    // add_const(sub(*as[v], *bs[i]), consts[v]) word for word, written straight into
    // the V B stack by one launch (k_sub_bounds_stacked: each bs[i] loaded once for
    // all bounds, the as' words once per tile of members).  sub_stacked's level
    // rules: as at a lower level than the bs are level-adjusted once, at a higher
    // one every member takes its own ops.  FHE_RUN_FUSED=0 (A/B): sub_stacked per
    // bound, then add_const in place.
    CtPtr sub_bounds_stacked(const std::vector<const Ciphertext *> &as, const std::vector<const Ciphertext *> &bs,
                             const std::vector<double> &consts);
    // the B-member stack a against the column-major stack b of P B members, all at
    // one level: member p B + z of the result is mul(add_const(member(a, z), c),
    // member(b, p B + z)) (mul_pairs_const) or mul(sub(member(a, z), member(a_sub, z)),
    // member(b, p B + z)) (mul_pairs_sub) word for word.  One tensor pass
    // (k_tensor_run: the left operand formed once per thread for up to four
    // columns, never written to memory), then mul's relinearisation / rescale
    // tail on P B members.  FHE_RUN_FUSED=0 (A/B): the left operand formed by
    // add_const / sub, then one mul per column, stacked.
    CtPtr mul_pairs_const(const Ciphertext &a, double c, const Ciphertext &b, int P);
    CtPtr mul_pairs_sub(const Ciphertext &a, const Ciphertext &a_sub, const Ciphertext &b, int P);
    // the two above: a_sub null takes the constant
    CtPtr mul_pairs_left(const char *what, const Ciphertext &a, const Ciphertext *a_sub, double c, const Ciphertext &b,
                         int P);
    // The sign arguments of the window sums (DirectSortN::windowSums, DESIGN.md
    // §6.7): G = part_as.size() partition keys (1..3) against B shifted operands each
    // (part_bs key-major) and an optional order key against order_bs (B of them), as
    // one stack of (2 G + V) B members.  Members (2 g) B + i and (2 g + 1) B + i =
    // add_const(sub(*part_as[g], *part_bs[g B + i]), +eps resp. -eps).  Behind them the
    // order key's V B members: with ps, member 2 G B + i = add_plain(sub(*order_a,
    // *order_bs[i]), *ps[i]) (V = 1); with order_lo, members 2 G B + i =
    // add_const(sub(*order_a, .), +eps) and (2 G + 1) B + i = add_const(sub(*order_lo, .),
    // -eps) (V = 2); otherwise member 2 G B + i = add_const(sub(*order_a, .), order_const)
    // (V = 1); no order_a: V = 0.  Word for word, written by one launch
    // (k_sub_window_stacked: each operand loaded once, a left operand's words once
    // per tile of members).  sub_stacked's level rules: left operands (all at one
    // level) below the operands are level-adjusted once, above them every member
    // takes its own ops.  FHE_WIN_FUSED=0 (A/B): sub_stacked per side, then
    // add_const in place resp. add_plain per member.
    CtPtr sub_window_stacked(const std::vector<const Ciphertext *> &part_as,
                             const std::vector<const Ciphertext *> &part_bs, const Ciphertext *order_a,
                             const Ciphertext *order_lo, const std::vector<const Ciphertext *> &order_bs,
                             const std::vector<const Plaintext *> &ps, double order_const, double eps);
    // stacks of B members each, u and w at one level, u2 and w2 at one level: member
    // z = mul(sub(member(u, z), member(w, z)), sub(member(u2, z), member(w2, z))) word for
    // word.  With all four at one level it is one tensor pass that forms both
    // differences as it loads them (k_tensor_win), then mul's relinearisation /
    // rescale tail; with the pairs at two levels (mul would level-adjust one) or
    // under FHE_WIN_FUSED=0 it is sub, sub and the product.
    CtPtr mul_sub_sub(const Ciphertext &u, const Ciphertext &w, const Ciphertext &u2, const Ciphertext &w2);
    CtPtr sum_members(const Ciphertext &a);
    // acc[p] (+)= sum_z a[p B + z] for the `groups` groups of B = a.batch / groups
    // consecutive members, in one launch (k_sum_member_groups); an empty acc
    // receives the sums, an exclusively owned one of the same level is added to
    // in place.  FHE_SORT_COLS_FUSED=0 (A/B): one sum_members per group, stacked.
    void sum_member_groups(const Ciphertext &a, int groups, CtPtr &acc);
    // sum over ranks already done into ct (u64 add, no reduction): reduce mod q
    void reduce_after_allreduce(Ciphertext &ct);

    // ---------------------------------------------- kernel-level access ---
    // host in/out, for parity tests
    void ntt_host(u64 *data, int prime_index, int limbs, bool inverse);
    void modup_host(const u64 *d, size_t ell, u64 *ext);          // ext [digits][ell+K][n] NTT
    void moddown_host(const u64 *in, size_t ell, u64 *out);        // in [ell+K][n] -> [ell][n]
    void automorph_host(const u64 *in, size_t limbs, u64 g, u64 *out);
    // device-resident variants: enqueued on `stream` (nullptr:
    // the engine stream), no host synchronisation.  ntt_dev transforms `limbs`
    // consecutive-prime limbs of `segments` polynomials in place (segment s at
    // data + s * seg_stride); automorph_dev writes in[...] o X -> X^g (NTT form).
    void ntt_dev(u64 *data, int prime_index, int limbs, int segments, size_t seg_stride, bool inverse, void *stream);
    void automorph_dev(const u64 *in, u64 *out, size_t limbs, u64 g, void *stream);
    // time `iters` back-to-back launches of one kernel on the engine stream
    // (HIP events), shaped like a key switch at `limbs` Q limbs; returns the
    // average ms per launch and the algorithmic HBM bytes per launch.
    void time_kernel(const std::string &name, size_t limbs, int iters, double &avg_ms, double &bytes);
    // live per-launch clock over real work: between start and stop every NTT
    // pass is bracketed by HIP events on the engine stream; stop() returns JSON
    // {"kernel": {"launches": c, "ms": total, "bytes": total_algorithmic}, ...}
    // device pool: release cached blocks; bytes live / cached / peak live
    // process-wide host costs: {encodes, encode seconds, pool-miss hipMallocs,
    // hipMalloc seconds} (the cold-sort breakdown)
    static void host_stats_get(double out[4]);
    static void host_stats_reset();
    void pool_trim();
    void pool_stats(size_t &live, size_t &cached, size_t &peak) const;
    void kernel_clock_start();
    std::string kernel_clock_stop();
    // algorithm phase the clocked kernels and op bytes are booked under
    // (nullptr = none); returns the previous one
    static const char *set_algo_phase(const char *phase);

    // small device scratch (for collectives / headers); copies are synchronous
    struct DevBuf {
        std::shared_ptr<DevMem> mem;
        u64 *ptr = nullptr;
    };
    DevBuf alloc_u64(size_t count);
    void h2d(u64 *dst, const u64 *src, size_t count);
    void d2h(u64 *dst, const u64 *src, size_t count);

    void sync();
    void *stream_handle();   // hipStream_t
    int device() const;
    Counters ctr;

    struct Impl;
    std::unique_ptr<Impl> impl;

  private:
    struct ForkTag {};
    explicit Engine(ForkTag);

  private:
    std::shared_ptr<int> ps_split_ = std::make_shared<int>(PS_SPLIT_OPENFHE);
    CtPtr new_ct(int level, int slots, double scale, size_t limbs, int batch = 1);
    // what the stacked products share behind their own tensor pass (engine.hip)
    template <class Tensor>
    CtPtr product_tail(const Ciphertext &a, int members, Tensor &&tensor);
    std::vector<CtPtr> linear_sums_run(const std::vector<const Ciphertext *> &xs, const int64_t *K, const uint8_t *sh,
                                       const int64_t *Kc, const uint8_t *shc, size_t G, int target, bool rescale,
                                       const char *who);
};

// Raised on a rotation index with no key (the reference's OpenFHE raises on
// EvalRotate with a missing key).
struct NoKeyError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

}  // namespace fhe
