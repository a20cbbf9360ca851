// MI355X RNS-CKKS engine: device residency, tables, keys and op orchestration.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <stdexcept>
#include <functional>
#include <thread>

#include "../device/kernels.hpp"
#include "engine.hpp"

#define HIP_OK(x)                                                                                     \
    do {                                                                                              \
        hipError_t _e = (x);                                                                          \
        if (_e != hipSuccess)                                                                         \
            throw std::runtime_error(std::string("HIP error ") + hipGetErrorString(_e) + " at " +    \
                                     __FILE__ + ":" + std::to_string(__LINE__));                      \
    } while (0)

namespace fhe {

using dev::Mod;

// ================================================================ pool ====
// Every engine (and every fork: concurrent sort lanes) owns a pool; an
// allocation that fails first releases the cached blocks of all pools of the
// process, so one lane's cache never starves another lane or a later phase.
// process-wide host-side cost counters (cold-start breakdown, fhe_host_stats):
// host encodes (special FFT + rounding + upload + NTT, until the plaintext is
// complete) and device allocations that missed the pool's cache
struct HostStats {
    std::atomic<u64> encode_ns{0}, encodes{0}, malloc_ns{0}, mallocs{0};
};
HostStats &host_stats() {
    static HostStats h;
    return h;
}
u64 now_ns() {
    return (u64)std::chrono::duration_cast<std::chrono::nanoseconds>(
               std::chrono::steady_clock::now().time_since_epoch())
        .count();
}

struct Pool;
std::mutex &pool_registry_mu() {
    static std::mutex m;
    return m;
}
std::set<Pool *> &pool_registry() {
    static std::set<Pool *> r;
    return r;
}
void trim_all_pools();

// Allocation size classes: 256-B granules up to 1 MiB, above that 8 classes
// per power of two (<= 12.5% slack).  Ciphertext batches come in many limb
// counts x member counts; with exact sizes every new shape missed the cache
// and cost a hipMalloc (MEHP24 at ring 2^17 cached 135 GB of odd sizes).
inline size_t size_class(size_t bytes) {
    if (bytes <= ((size_t)1 << 20)) return (bytes + 255) & ~(size_t)255;
    int top = 63 - __builtin_clzll((unsigned long long)bytes);
    const size_t step = (size_t)1 << (top - 3);
    return (bytes + step - 1) & ~(step - 1);
}

struct Pool {
    Pool() {
        std::lock_guard<std::mutex> lk(pool_registry_mu());
        pool_registry().insert(this);
    }
    Pool(const Pool &) = delete;
    std::mutex mu;
    std::multimap<size_t, void *> free_list;
    size_t live = 0, cached = 0, peak = 0;
    int device = 0;
    // Best fit: the smallest cached block of at least `bytes` is reused if it is
    // no more than 1.5x the request (its real size is returned in `bytes`, to be
    // handed back to put), else a new class-sized block is allocated.
    void *get(size_t &bytes) {
        bytes = size_class(bytes);
        {
            std::lock_guard<std::mutex> lk(mu);
            auto it = free_list.lower_bound(bytes);
            if (it != free_list.end() && it->first <= bytes + bytes / 2) {
                void *p = it->second;
                bytes = it->first;
                free_list.erase(it);
                cached -= bytes;
                live += bytes;
                peak = std::max(peak, live);
                return p;
            }
        }
        void *p = nullptr;
        const u64 t0 = now_ns();
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) {
            trim_all_pools();
            HIP_OK(hipMalloc(&p, bytes));
        }
        host_stats().malloc_ns += now_ns() - t0;
        host_stats().mallocs++;
        std::lock_guard<std::mutex> lk(mu);
        live += bytes;
        peak = std::max(peak, live);
        return p;
    }
    void put(void *p, size_t bytes) {  // bytes: the block size get() returned
        std::lock_guard<std::mutex> lk(mu);
        free_list.emplace(bytes, p);
        live -= bytes;
        cached += bytes;
    }
    void trim() {
        std::lock_guard<std::mutex> lk(mu);
        (void)hipDeviceSynchronize();
        for (auto &kv : free_list) (void)hipFree(kv.second);
        free_list.clear();
        cached = 0;
    }
    ~Pool() {
        {
            std::lock_guard<std::mutex> lk(pool_registry_mu());
            pool_registry().erase(this);
        }
        for (auto &kv : free_list) (void)hipFree(kv.second);
    }
};
void trim_all_pools() {
    std::lock_guard<std::mutex> lk(pool_registry_mu());
    for (Pool *p : pool_registry()) p->trim();
}

struct DevMem {
    std::shared_ptr<Pool> pool;
    void *p = nullptr;
    size_t bytes = 0;
    ~DevMem() {
        if (p) pool->put(p, bytes);
    }
};

// ================================================================ impl ====
// tags the NTT launches of one engine helper in the live kernel clock
struct Phase {
    const char *prev;
    explicit Phase(const char *p) : prev(dev::launch_phase()) { dev::launch_phase() = p; }
    ~Phase() { dev::launch_phase() = prev; }
};

struct Engine::Impl {
    host::Params P;
    host::LevelTables LT;
    int device = 0;
    hipStream_t st = nullptr;
    std::shared_ptr<Pool> pool;
    u64 seed = 0;
    host::Entropy ent;  // sampling keys: deterministic streams for seed != 0, else getrandom
    // encryption-randomness stream index, shared with forked engines so no
    // two encryptions under one context ever reuse (v, e0, e1)
    std::shared_ptr<std::atomic<u64>> enc_counter = std::make_shared<std::atomic<u64>>(0);

    // static device tables
    std::vector<std::shared_ptr<DevMem>> keep;
    Mod *mods = nullptr;
    dev::NttTables T{};
    int *extmap = nullptr;   // [nq+1][nq+K]
    int *iota = nullptr;     // [nall]: 0, 1, 2, ... (prime maps of consecutive primes)
    u64 *modup_tab = nullptr;  // packed ModUp tables
    u64 *phinv = nullptr, *phinv_s = nullptr, *phat = nullptr, *pinv = nullptr, *pinv_s = nullptr;
    u64 *qlinv = nullptr, *qlinv_s = nullptr;
    u64 *pmod = nullptr, *pmod_s = nullptr, *pqlinv = nullptr, *pqlinv_s = nullptr;
    double *pinvd = nullptr;
    double *mdfp_c = nullptr, *mdfp_q = nullptr;  // fp64 ModDown + rescale rows (LevelTables)
    double *modup_fp = nullptr;  // fp64 ModUp rows (LevelTables modup_fp)
    int *modup_smap = nullptr, *modup_pmap = nullptr;
    // the NTT's host-side class table (T.fp_host points into it) and the prime
    // maps registered with the NTT launcher; shared with forks, released (maps
    // unregistered) with the last engine holding the tables
    struct FpState {
        std::vector<uint8_t> fp_host;
        std::vector<const int *> maps;
        void reg(const int *dev, const std::vector<int> &host) {
            dev::ntt_register_map(dev, host.data(), host.size());
            maps.push_back(dev);
        }
        ~FpState() {
            for (const int *m : maps) dev::ntt_unregister_map(m);
        }
    };
    std::shared_ptr<FpState> fps = std::make_shared<FpState>();

    // keys
    // key material, shared by an engine and its forks (sort lanes): a key load
    // on the parent replaces the members in place, so every fork sees it
    struct KeySet {
        std::shared_ptr<DevMem> s_ntt, pk, relin;
        std::map<u64, std::shared_ptr<DevMem>> rotkeys;
        // public stream v1 (csrc/wire/wire.hpp): the seed keygen expands the
        // switching keys' uniform halves from, when set, and the seed of every
        // key whose a halves are that stream (kid 0 = relin, else the galois
        // element); a key loaded in full is in no entry
        bool has_pub_seed = false;
        PublicSeed pub_seed{};
        std::map<u64, PublicSeed> seeded;
    };
    std::shared_ptr<DevMem> pub_err;  // the expansion kernel's error word
    std::shared_ptr<KeySet> ks = std::make_shared<KeySet>();
    std::map<u64, std::shared_ptr<DevMem>> perms;
    int key_digits = 0;

    // device copies of the leaf sums' constant tables ([G][m] K and shift),
    // keyed by their bytes: a series at a level uploads once per engine (first
    // sort), the sums read them from HBM (kernels.hip k_leaf_sums_mfma)
    struct ConstTab {
        std::shared_ptr<DevMem> mem;
        std::vector<int64_t> K;  // host copies stay alive for the asynchronous upload
        std::vector<uint8_t> sh;
        u64 used = 0;
    };
    std::map<std::string, ConstTab> ctabs;
    u64 ctab_tick = 0;
    std::pair<const int64_t *, const uint8_t *> const_table(const std::vector<int64_t> &K,
                                                           const std::vector<uint8_t> &sh) {
        std::string key(reinterpret_cast<const char *>(K.data()), K.size() * sizeof(int64_t));
        key.append(reinterpret_cast<const char *>(sh.data()), sh.size());
        key.append(std::to_string(K.size()));
        auto it = ctabs.find(key);
        if (it == ctabs.end()) {
            if (ctabs.size() >= 4096) {  // bound the cache: drop the least recently used
                auto lru = ctabs.begin();
                for (auto j = ctabs.begin(); j != ctabs.end(); ++j)
                    if (j->second.used < lru->second.used) lru = j;
                HIP_OK(hipStreamSynchronize(st));  // its upload / readers are done
                ctabs.erase(lru);
            }
            ConstTab t;
            t.K = K;
            t.sh = sh;
            const size_t kb = K.size() * sizeof(int64_t);
            t.mem = alloc(kb + sh.size());
            HIP_OK(hipMemcpyAsync(t.mem->p, t.K.data(), kb, hipMemcpyHostToDevice, st));
            HIP_OK(hipMemcpyAsync(static_cast<char *>(t.mem->p) + kb, t.sh.data(), sh.size(), hipMemcpyHostToDevice, st));
            it = ctabs.emplace(std::move(key), std::move(t)).first;
        }
        it->second.used = ++ctab_tick;
        const char *b = static_cast<const char *>(it->second.mem->p);
        return {reinterpret_cast<const int64_t *>(b), reinterpret_cast<const uint8_t *>(b + K.size() * sizeof(int64_t))};
    }

    // device copies of mul_plain_sum_batches' plaintext pointer tables ([nb][m]),
    // keyed by their bytes like the constant tables: the rank's masks are cached
    // plaintexts, so a sort after the first finds its table and uploads nothing
    struct PtrTab {
        std::shared_ptr<DevMem> mem;
        std::vector<const u64 *> host;  // stays alive for the asynchronous upload
        u64 used = 0;
    };
    std::map<std::string, PtrTab> ptabs;
    const u64 *const *ptr_table(const std::vector<const u64 *> &v) {
        std::string key(reinterpret_cast<const char *>(v.data()), v.size() * sizeof(const u64 *));
        auto it = ptabs.find(key);
        if (it == ptabs.end()) {
            if (ptabs.size() >= 256) {
                auto lru = ptabs.begin();
                for (auto j = ptabs.begin(); j != ptabs.end(); ++j)
                    if (j->second.used < lru->second.used) lru = j;
                HIP_OK(hipStreamSynchronize(st));
                ptabs.erase(lru);
            }
            PtrTab t;
            t.host = v;
            t.mem = alloc(v.size() * sizeof(const u64 *));
            HIP_OK(hipMemcpyAsync(t.mem->p, t.host.data(), v.size() * sizeof(const u64 *), hipMemcpyHostToDevice, st));
            it = ptabs.emplace(std::move(key), std::move(t)).first;
        }
        it->second.used = ++ctab_tick;
        return static_cast<const u64 *const *>(it->second.mem->p);
    }

    // device encoder tables (the host encoder's ksi / rot, uploaded on first use)
    const double2 *enc_ksi = nullptr;
    const uint32_t *enc_rot = nullptr;
    void enc_tables() {
        if (enc_ksi) return;
        std::vector<double> ksi;
        std::vector<uint32_t> rot;
        host::embedding_tables(P.n, ksi, rot);
        enc_ksi = reinterpret_cast<const double2 *>(upload_static(ksi));
        enc_rot = upload_static(rot);
    }
    // v [B][S] slot values on the device, member order sorted by level:
    // plaintexts (one allocation per level, member views) in that order
    std::vector<PtPtr> encode_sorted(double2 *v, int B, int S, const std::vector<int> &levels,
                                     const std::vector<double> &scales) {
        const size_t nn = n();
        auto coefm = alloc((size_t)B * nn * 8);
        int64_t *coef = static_cast<int64_t *>(coefm->p);
        auto scm = alloc((size_t)B * 8 + 8);
        double *sc = static_cast<double *>(scm->p);
        unsigned *ovf = reinterpret_cast<unsigned *>(sc + B);
        HIP_OK(hipMemcpyAsync(sc, scales.data(), (size_t)B * 8, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemsetAsync(ovf, 0, 4, st));
        dev::encode_ifft(v, coef, B, S, (int)nn, enc_ksi, enc_rot, sc, ovf, st);
        std::vector<PtPtr> out(B);
        for (int a = 0; a < B;) {
            int b = a;
            while (b < B && levels[b] == levels[a]) ++b;
            const size_t ell = P.limbs_at(levels[a]);
            auto blk = alloc((size_t)(b - a) * ell * nn * 8);
            u64 *d = static_cast<u64 *>(blk->p);
            dev::ew_signed_to_rns(d, coef + (size_t)a * nn, (int)ell, nullptr, mods, P.logN, st, b - a, ell * nn, nn);
            dev::ntt_forward(d, (int)ell, b - a, ell * nn, nullptr, T, st);
            for (int i = a; i < b; ++i) {
                auto pt = std::make_shared<Plaintext>();
                pt->mem = blk;
                pt->data = d + (size_t)(i - a) * ell * nn;
                pt->level = levels[a];
                pt->slots = S;
                pt->scale = scales[i];
                pt->limbs = ell;
                out[i] = pt;
            }
            a = b;
        }
        unsigned flag = 0;
        HIP_OK(hipMemcpyAsync(&flag, ovf, 4, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));  // also: the scale table's host source outlives its copy
        if (flag) throw std::overflow_error("encode: scaled coefficient exceeds 63 bits");
        return out;
    }

    std::shared_ptr<DevMem> alloc(size_t bytes) {
        auto m = std::make_shared<DevMem>();
        m->pool = pool;
        m->p = pool->get(bytes);  // bytes becomes the block size
        m->bytes = bytes;
        return m;
    }
    template <class T>
    T *upload_static(const std::vector<T> &v) {
        auto m = alloc(std::max<size_t>(v.size(), 1) * sizeof(T));
        HIP_OK(hipMemcpy(m->p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
        keep.push_back(m);
        return static_cast<T *>(m->p);
    }
    size_t n() const { return P.n; }
    size_t wmax() const { return P.nq() + P.K; }
    const int *ext(size_t ell) const { return extmap + ell * wmax(); }
    const uint32_t *perm(u64 g) {
        auto it = perms.find(g);
        if (it != perms.end()) return static_cast<const uint32_t *>(it->second->p);
        auto v = host::automorphism_perm(P.logN, g);
        auto m = alloc(v.size() * 4);
        HIP_OK(hipMemcpyAsync(m->p, v.data(), v.size() * 4, hipMemcpyHostToDevice, st));
        HIP_OK(hipStreamSynchronize(st));
        perms[g] = m;
        return static_cast<const uint32_t *>(m->p);
    }

    // ------------------------------------------------------- key switch --
    // Every helper works on `members` independent polynomials at once (a
    // ciphertext batch): member m of an input sits at m * stride.
    //
    // ext[m][j][t] (NTT form) for all digits of d[m] ([ell][n], NTT form)
    // FHE_KS_FUSE (A/B, default 1; 548.2 -> 537.8 ms, profiles/r5_g): the relinearisation runs ModUp's forward row
    // pass fused with the key-switch inner product for the FP-class targets
    // (dev::ntt_row_ks; integer targets keep the row pass + ks_inner)
    bool ks_fuse(int members) const {
        static const bool on = env_switch("FHE_KS_FUSE", 1);
        // FHE_KS_FUSE_MIN (A/B): the fewest members a fused launch takes (default 4)
        static const int min_members = std::max(1, env_switch("FHE_KS_FUSE_MIN", 4));
        return on && members >= min_members && (P.logN == 16 || P.logN == 17);
    }
    // FHE_KS_FUSE_INT (A/B, default 1; round 6, verdict r5 item 2): the integer-class
    // targets (q_0, the special primes) through the fused kernel too -- ModUp then
    // runs no row pass at all and ks_inner none: sort 516.5 / 517.3 -> 509.9 / 510.6 ms
    // (profiles/r6_ab/ks_fuse_int_ab.jsonl); round 5 had measured the fused integer
    // launch per target against the FP one, not against the row pass + ks_inner it replaces
    static bool ks_fuse_int() {
        static const bool on = env_switch("FHE_KS_FUSE_INT", 1);
        return on;
    }
    // FHE_MULTAIL_OWN (A/B, default 1): a one-digit HMult (ell <= alpha; 124 of the
    // N=1024 sort's 162 stacked HMults) leaves the own-digit key product of its Q
    // limbs below ell - 1 to the closing row pass (k_ntt_fwd_row<5, ...>) instead of
    // storing it from k_ntt_row_ks and reading it back; 0: the accumulator path
    static bool multail_own() {
        static const bool on = env_switch("FHE_MULTAIL_OWN", 1);
        return on;
    }
    // cols_only: the forward NTT's column pass alone (the row pass runs fused
    // with the key switch, mul_tail)
    std::shared_ptr<DevMem> modup(const u64 *d, size_t ell, int members, size_t d_stride, bool cols_only = false) {
        Phase phase_("modup");
        const size_t nn = n(), K = (size_t)P.K, W = ell + K;
        const int digits = P.digits_at(ell);
        auto coef = alloc((size_t)members * ell * nn * 8);
        u64 *c = static_cast<u64 *>(coef->p);
        dev::ntt_inverse_from(c, d, d_stride, (int)ell, members, ell * nn, nullptr, T, st, /*raw*/ true);
        const size_t es = (size_t)digits * W * nn;
        auto extm = alloc((size_t)members * es * 8);
        u64 *e = static_cast<u64 *>(extm->p);
        dev::modup_convert(e, c, (int)ell, P.K, P.alpha, digits, members, ell * nn, es, ext(ell), modup_tab,
                           LT.modup_off[ell].data(), mods, P.logN, st, modup_fp, LT.modup_fp_off[ell].data(),
                           LT.modup_fp_mid);
        const size_t mo = LT.modup_map_off[ell];
        if (cols_only) {
            // the column pass for every limb; the row pass here only for the
            // integer-class primes (the FP targets' row pass runs fused with the
            // inner product, mul_tail)
            const int cnt = (int)LT.modup_map_cnt[ell];
            dev::ntt_forward_mapped_cols(e, cnt, members, es, modup_smap + mo, modup_pmap + mo, T, st);
            if (!ks_fuse_int())
            for (auto &r : dev::ntt_class_runs(modup_pmap + mo, cnt, false, T))
                dev::ntt_forward_mapped_rows(e, r.second, members, es, modup_smap + mo + r.first,
                                             modup_pmap + mo + r.first, T, st);
        } else
            dev::ntt_forward_mapped(e, (int)LT.modup_map_cnt[ell], members, es, modup_smap + mo, modup_pmap + mo, T, st);
        return extm;
    }
    // rotation key switch: out[m] (= [2][ell][n]) = ModDown(sum_j ext_j * key_j) + (add[m], 0);
    // d: the switched polynomial of member m at m * d_stride (NTT form)
    void ks_apply(const u64 *e, const u64 *d, size_t d_stride, size_t ell, int members, const u64 *key,
                  const uint32_t *pm, u64 *out, const u64 *add, size_t add_stride) {
        Phase phase_("ks_moddown");
        const size_t nn = n(), K = (size_t)P.K, W = ell + K;
        const int digits = P.digits_at(ell);
        const int segs = 2 * members;
        auto accm = alloc((size_t)segs * W * nn * 8);
        u64 *acc = static_cast<u64 *>(accm->p);
        dev::KsStrides str;
        str.acc = 2 * W * nn;
        str.ext = (size_t)digits * W * nn;
        str.d = d_stride;
        dev::ks_inner(acc, e, d, key, (int)ell, P.K, (int)P.nq(), (int)P.nall(), P.alpha, digits, pm, ext(ell), mods,
                      P.logN, st, members, str);
        ks_moddown(acc, ell, segs, out, add, add_stride);
    }
    // ModDown of `segs` accumulators acc [segs][ell+K][n] (NTT form): out[s] =
    // ModDown(acc[s]) (+ add[s / 2] on the c0 segments)
    void ks_moddown(u64 *acc, size_t ell, int segs, u64 *out, const u64 *add, size_t add_stride) {
        const size_t nn = n(), K = (size_t)P.K, W = ell + K;
        dev::ntt_inverse(acc + ell * nn, (int)K, segs, W * nn, ext(ell) + ell, T, st, /*raw*/ true);
        auto convm = alloc((size_t)segs * ell * nn * 8);
        u64 *conv = static_cast<u64 *>(convm->p);
        dev::moddown_convert(conv, acc + ell * nn, (int)ell, P.K, (int)P.nq(), W * nn, ell * nn, segs, phinv, phinv_s,
                             phat, pmod, pinvd, mods, P.logN, st);
        ks_finish(conv, acc, ell, segs, out, add, add_stride);
    }
    // `count` key switches in the same launches: switch m uses keys.key[m] and
    // reads its ext (stride e_stride; 0 = one hoisted ModUp shared by all)
    // through keys.perm[m]; out[m] ([2][ell][n]) = ModDown(acc_m) + (add[m], 0)
    void ks_apply_multi(const u64 *e, size_t e_stride, const u64 *d, size_t d_stride, size_t ell, int count,
                        const dev::KsKeys &keys, u64 *out, const u64 *add, size_t add_stride) {
        Phase phase_("ks_moddown");
        const size_t nn = n(), K = (size_t)P.K, W = ell + K;
        const int digits = P.digits_at(ell);
        const int segs = 2 * count;
        auto accm = alloc((size_t)segs * W * nn * 8);
        u64 *acc = static_cast<u64 *>(accm->p);
        dev::KsStrides str;
        str.acc = 2 * W * nn;
        str.ext = e_stride;
        str.d = d_stride;
        dev::ks_inner_multikey(acc, e, d, keys, count, (int)ell, P.K, (int)P.nall(), P.alpha, digits, ext(ell), mods,
                               P.logN, st, str);
        ks_moddown(acc, ell, segs, out, add, add_stride);
    }
    // out[s] = (acc[s] - NTT(conv[s])) P^-1 (+ add[s / 2] on c0): the forward NTT of
    // the converted special part whose row pass finishes the ModDown
    void ks_finish(u64 *conv, const u64 *acc, size_t ell, int segs, u64 *out, const u64 *add, size_t add_stride) {
        const size_t nn = n(), W = ell + (size_t)P.K;
        dev::NttFuse F;
        F.out = out;
        F.seg_out = ell * nn;
        F.x = acc;
        F.seg_x = W * nn;
        F.d = add;
        F.seg_d = add_stride;
        F.c1 = pinv;
        F.c1s = pinv_s;
        dev::ntt_forward_ksfinish(conv, (int)ell, segs, F, T, st);
    }
    // HMult tail, fused: out[m] ([2][ell-1][n]) = Rescale(d01[m] + ModDown(Sum_j ext_j * key_j)).
    // Bit-identical to a ModDown with d01 added followed by rescale(): both
    // compute ((acc - Conv(acc_P)) P^-1 + d - [y_last]) q_last^-1 mod q_i, but
    // here only limb ell-1 and the P limbs leave the NTT domain and one forward
    // NTT of ell-1 limbs per polynomial serves both divisions.
    // d01 [members][2][ell][n], d2 [members][ell][n] (NTT form).
    // fused: e is ModUp's output after the column pass only (modup cols_only)
    void mul_tail(const u64 *e, const u64 *d01, const u64 *d2, size_t ell, int members, u64 *out, bool fused = false) {
        Phase phase_("mul_tail");
        const size_t nn = n(), K = (size_t)P.K, W = ell + K;
        const int digits = P.digits_at(ell);
        const int segs = 2 * members;
        auto accm = alloc((size_t)segs * W * nn * 8);
        u64 *acc = static_cast<u64 *>(accm->p);
        dev::KsStrides str;
        str.acc = 2 * W * nn;
        str.ext = (size_t)digits * W * nn;
        str.d = ell * nn;
        dev::KsFold fold;
        fold.d = d01 + (ell - 1) * nn;
        fold.seg = ell * nn;
        fold.member = 2 * ell * nn;
        fold.w = LT.pmod[ell - 1];
        fold.ws = LT.pmod_s[ell - 1];
        // one digit (ell <= alpha): every Q limb is an own-digit limb, its accumulator
        // the element-wise product d2 * key.  The closing row pass forms that product
        // itself for the limbs below ell - 1 (ntt_forward_multail_own), so only
        // q_last (with the fold) and the special primes go through ntt_row_ks and
        // the Q rows of acc below ell - 1 are never written or read
        const bool own = fused && digits == 1 && ell >= 2 && ks_fuse_int() && multail_own();
        if (fused) {
            // FP targets: row pass + inner product fused; integer targets (q_0 and
            // the special primes): their row pass ran in modup, ks_inner here
            dev::ntt_row_ks(acc, e, d2, static_cast<u64 *>(ks->relin->p), (int)ell, P.K, (int)P.nall(), P.alpha, digits,
                            ext(ell), members, str, fold, T, st, /*fp_only*/ !ks_fuse_int(),
                            /*tfirst*/ own ? (int)ell - 1 : 0);
            const auto runs = ks_fuse_int() ? std::vector<std::pair<int, int>>{}
                                            : dev::ntt_class_runs(ext(ell), (int)W, false, T);
            for (size_t r = 0; r < runs.size(); r += 2) {
                dev::KsStrides s2 = str;
                s2.zs0 = runs[r].first;
                s2.zn0 = runs[r].second;
                s2.zs1 = r + 1 < runs.size() ? runs[r + 1].first : 0;
                const int cnt = runs[r].second + (r + 1 < runs.size() ? runs[r + 1].second : 0);
                dev::ks_inner(acc, e, d2, static_cast<u64 *>(ks->relin->p), (int)ell, P.K, (int)P.nq(), (int)P.nall(),
                              P.alpha, digits, nullptr, ext(ell), mods, P.logN, st, members, s2, fold, cnt);
            }
        } else
            dev::ks_inner(acc, e, d2, static_cast<u64 *>(ks->relin->p), (int)ell, P.K, (int)P.nq(), (int)P.nall(),
                          P.alpha, digits, nullptr, ext(ell), mods, P.logN, st, members, str, fold);
        dev::ntt_inverse(acc + (ell - 1) * nn, (int)K + 1, segs, W * nn, ext(ell) + (ell - 1), T, st, /*raw*/ true);
        auto corrm = alloc((size_t)segs * (ell - 1) * nn * 8);
        u64 *corr = static_cast<u64 *>(corrm->p);
        dev::moddown_rescale_convert(corr, acc, (int)ell, P.K, (int)P.nq(), W * nn, (ell - 1) * nn, segs, phinv,
                                     phinv_s, phat, pinv, pinv_s, pmod, pinvd, T.ninv, T.ninv_s, mods, P.logN, st,
                                     pmod_s, mdfp_c, mdfp_q, LT.mdfp_mid);
        // forward NTT of corr whose row pass finishes (acc + d P - corr) (P q_last)^-1 into `out`
        dev::NttFuse F;
        F.out = out;
        F.seg_out = (ell - 1) * nn;
        F.x = acc;
        F.seg_x = W * nn;
        F.d = d01;
        F.seg_d = ell * nn;
        F.c1 = pqlinv + ell * P.nq();
        F.c1s = pqlinv_s + ell * P.nq();
        F.c2 = pmod;
        F.c2s = pmod_s;
        if (own) {
            F.x = nullptr;
            F.d2 = d2;
            F.seg_d2 = ell * nn;
            F.key = static_cast<const u64 *>(ks->relin->p);
            F.nall = (int)P.nall();
            dev::ntt_forward_multail_own(corr, (int)(ell - 1), segs, F, T, st);
            return;
        }
        dev::ntt_forward_multail(corr, (int)(ell - 1), segs, F, T, st);
    }
    // out [segs][ell-1][n] = Rescale(K * in) from the first ell limbs of
    // in [segs][.][n] (segment stride seg_in); K = 0 means no scalar
    void rescale(const u64 *in, size_t ell, size_t seg_in, int segs, u64 *out, host::SConst K = {}) {
        Phase phase_("rescale");
        const size_t nn = n();
        auto lastm = alloc((size_t)segs * nn * 8);
        u64 *last = static_cast<u64 *>(lastm->p);
        dev::ntt_inverse_from(last, in + (ell - 1) * nn, seg_in, 1, segs, nn, ext(ell) + (ell - 1), T, st);
        if (ell <= 1) return;
        auto tmpm = alloc((size_t)segs * (ell - 1) * nn * 8);
        u64 *tmp = static_cast<u64 *>(tmpm->p);
        // column pass lifts `last` into every prime on load; row pass finishes
        // (in - NTT(lift)) q_last^-1 straight into `out`
        dev::NttFuse F;
        F.last = last;
        F.seg_last = nn;
        F.lastp = (int)(ell - 1);
        F.out = out;
        F.seg_out = (ell - 1) * nn;
        F.x = in;
        F.seg_x = seg_in;
        F.c1 = qlinv + ell * P.nq();
        F.c1s = qlinv_s + ell * P.nq();
        F.scalar = K.k;
        F.scalar_sh = K.sh;
        dev::ntt_forward_rescale(tmp, (int)(ell - 1), segs, F, T, st);
    }
};

// ============================================================== engine ====
Engine::Engine(int logN, int L, int scale_bits, int first_bits, int dnum, int device, u64 seed)
    : impl(new Impl) {
    auto &I = *impl;
    I.device = device;
    I.seed = seed;
    // refuses a context outside the kernels' envelope (digits, digit width,
    // special primes, ring) before the device is touched
    I.P = host::envelope_params(logN, L, scale_bits, first_bits, dnum);
    I.ent = host::Entropy::from_seed(seed);
    dev::install_fault_report();  // FHE_FAULT_REPORT=1 only
    HIP_OK(hipSetDevice(device));
    HIP_OK(hipStreamCreateWithFlags(&I.st, hipStreamNonBlocking));
    I.pool = std::make_shared<Pool>();
    I.pool->device = device;
    I.LT = host::make_level_tables(I.P);
    // kernel preconditions: basis conversions hold <= 16 source residues in
    // registers and accumulate 30-bit-split products of residues < 2^60
    for (u64 q : I.P.primes)
        if (q >> 60) throw std::invalid_argument("engine: every prime must be < 2^60 (first_bits <= 60)");
    // rescales lift the last limb with a compare-select: every prime that can be
    // rescaled away (q_1..q_L) must satisfy q_l / 2 < q_i for all Q primes
    {
        u64 qmin = ~0ull, qlmax = 0;
        for (size_t i = 0; i < I.P.nq(); ++i) qmin = std::min(qmin, I.P.primes[i]);
        for (size_t i = 1; i < I.P.nq(); ++i) qlmax = std::max(qlmax, I.P.primes[i]);
        if (qlmax / 2 >= qmin) throw std::invalid_argument("engine: scaling primes must be < 2 x the smallest prime");
    }
    const size_t nall = I.P.nall(), n = I.P.n;
    std::vector<Mod> mods(nall);
    for (size_t i = 0; i < nall; ++i) {
        host::Modulus m(I.P.primes[i]);
        const u64 r64 = (u64)(((unsigned __int128)1 << 64) % m.q);
        mods[i] = Mod{m.q, m.mu, m.k, 0, r64, host::shoup(r64, m.q)};
    }
    I.mods = I.upload_static(mods);
    std::vector<u64> fwd(2 * nall * n), inv(2 * nall * n), ninv(nall), ninv_s(nall);
    // fp64 twiddles of the primes < 2^41 (the FP NTT launches; zero for the others)
    std::vector<double> fwdd(nall * n, 0.0), invd(nall * n, 0.0);
    std::vector<double2> qd(nall);
    std::vector<uint8_t> &fph = I.fps->fp_host;
    fph.assign(nall, 0);
    for (size_t i = 0; i < nall; ++i) {
        const u64 q = I.P.primes[i];
        fph[i] = dev::ntt_fp_prime(q) ? 1 : 0;
        qd[i] = make_double2((double)q, 1.0 / (double)q);
    }
    {
        std::vector<std::thread> th;
        const unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
        for (unsigned w = 0; w < nt; ++w)
            th.emplace_back([&, w]() {
                for (size_t i = w; i < nall; i += nt) {
                    auto t = host::make_ntt_table(I.P.primes[i], logN);
                    for (size_t k = 0; k < n; ++k) {  // interleaved {w, w'} pairs: one 16-B load
                        fwd[2 * (i * n + k)] = t.fwd[k];
                        fwd[2 * (i * n + k) + 1] = t.fwd_s[k];
                        inv[2 * (i * n + k)] = t.inv[k];
                        inv[2 * (i * n + k) + 1] = t.inv_s[k];
                        if (fph[i]) {
                            fwdd[i * n + k] = (double)t.fwd[k];
                            invd[i * n + k] = (double)t.inv[k];
                        }
                    }
                    ninv[i] = t.ninv;
                    ninv_s[i] = t.ninv_s;
                }
            });
        for (auto &t : th) t.join();
    }
    I.T.fwd2 = reinterpret_cast<const ulonglong2 *>(I.upload_static(fwd));
    I.T.inv2 = reinterpret_cast<const ulonglong2 *>(I.upload_static(inv));
    I.T.ninv = I.upload_static(ninv);
    I.T.ninv_s = I.upload_static(ninv_s);
    I.T.mods = I.mods;
    I.T.logN = logN;
    I.T.fwdd = I.upload_static(fwdd);
    I.T.invd = I.upload_static(invd);
    I.T.qd = I.upload_static(qd);
    I.T.fp_host = fph.data();
    I.extmap = I.upload_static(I.LT.extmap);
    I.fps->reg(I.extmap, I.LT.extmap);
    {
        std::vector<int> io(I.P.nall());
        for (size_t i = 0; i < io.size(); ++i) io[i] = (int)i;
        I.iota = I.upload_static(io);
        I.fps->reg(I.iota, io);
    }
    I.modup_tab = I.upload_static(I.LT.modup);
    I.phinv = I.upload_static(I.LT.phinv);
    I.phinv_s = I.upload_static(I.LT.phinv_s);
    I.phat = I.upload_static(I.LT.phat);
    I.pinv = I.upload_static(I.LT.pinv);
    I.pinv_s = I.upload_static(I.LT.pinv_s);
    I.qlinv = I.upload_static(I.LT.qlinv);
    I.qlinv_s = I.upload_static(I.LT.qlinv_s);
    I.pmod = I.upload_static(I.LT.pmod);
    I.pinvd = I.upload_static(I.LT.pinvd);
    I.mdfp_c = I.upload_static(I.LT.mdfp_c);
    I.mdfp_q = I.upload_static(I.LT.mdfp_q);
    I.modup_fp = I.upload_static(I.LT.modup_fp);
    // the ModUp forward NTT's limbs (every digit's targets) in any order: FP
    // primes first, so the launch splits into one FP and one integer run
    for (size_t ell = 1; ell <= I.P.nq(); ++ell) {
        const size_t o = I.LT.modup_map_off[ell], c = I.LT.modup_map_cnt[ell];
        std::vector<std::pair<int, int>> e(c);
        for (size_t y = 0; y < c; ++y) e[y] = {I.LT.modup_smap[o + y], I.LT.modup_pmap[o + y]};
        std::stable_partition(e.begin(), e.end(), [&](const std::pair<int, int> &v) { return fph[v.second] != 0; });
        for (size_t y = 0; y < c; ++y) {
            I.LT.modup_smap[o + y] = e[y].first;
            I.LT.modup_pmap[o + y] = e[y].second;
        }
    }
    I.modup_smap = I.upload_static(I.LT.modup_smap);
    I.modup_pmap = I.upload_static(I.LT.modup_pmap);
    I.fps->reg(I.modup_pmap, I.LT.modup_pmap);
    I.pmod_s = I.upload_static(I.LT.pmod_s);
    I.pqlinv = I.upload_static(I.LT.pqlinv);
    I.pqlinv_s = I.upload_static(I.LT.pqlinv_s);
    I.key_digits = I.P.digits_at(I.P.nq());
}

Engine::Engine(ForkTag) {}

std::unique_ptr<Engine> Engine::fork() const {
    std::unique_ptr<Engine> e(new Engine(ForkTag{}));
    e->ps_split_ = ps_split_;  // shared, not copied
    e->impl.reset(new Impl(*impl));  // shares tables and keys (shared_ptr / raw device pointers)
    auto &I = *e->impl;
    HIP_OK(hipSetDevice(I.device));
    I.st = nullptr;
    HIP_OK(hipStreamCreateWithFlags(&I.st, hipStreamNonBlocking));
    I.pool = std::make_shared<Pool>();
    I.pool->device = I.device;
    return e;
}

void Engine::wait_for(const Engine &other) {
    hipEvent_t ev;
    HIP_OK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    HIP_OK(hipEventRecord(ev, other.impl->st));
    HIP_OK(hipStreamWaitEvent(impl->st, ev, 0));
    HIP_OK(hipEventDestroy(ev));
}

Engine::~Engine() {
    if (impl && impl->st) {
        (void)hipStreamSynchronize(impl->st);
        impl->ks.reset();  // the last engine sharing the key set frees it
        impl->perms.clear();
        impl->keep.clear();
        (void)hipStreamDestroy(impl->st);
    }
}

const host::Params &Engine::params() const { return impl->P; }
size_t Engine::n() const { return impl->P.n; }
double Engine::delta(int level) const { return impl->P.delta[level]; }
void Engine::sync() { HIP_OK(hipStreamSynchronize(impl->st)); }
Engine::DevBuf Engine::alloc_u64(size_t count) {
    DevBuf b;
    b.mem = impl->alloc(std::max<size_t>(count, 1) * 8);
    b.ptr = static_cast<u64 *>(b.mem->p);
    return b;
}
void Engine::h2d(u64 *dst, const u64 *src, size_t count) {
    HIP_OK(hipMemcpyAsync(dst, src, count * 8, hipMemcpyHostToDevice, impl->st));
    HIP_OK(hipStreamSynchronize(impl->st));
}
void Engine::d2h(u64 *dst, const u64 *src, size_t count) {
    HIP_OK(hipMemcpyAsync(dst, src, count * 8, hipMemcpyDeviceToHost, impl->st));
    HIP_OK(hipStreamSynchronize(impl->st));
}
void *Engine::stream_handle() { return impl->st; }
int Engine::device() const { return impl->device; }

CtPtr Engine::new_ct(int level, int slots, double scale, size_t limbs, int batch) {
    if (batch < 1) throw std::invalid_argument("ciphertext batch must be >= 1");
    auto c = std::make_shared<Ciphertext>();
    c->mem = impl->alloc(2 * (size_t)batch * limbs * n() * 8);
    c->batch = batch;
    c->data = static_cast<u64 *>(c->mem->p);
    c->level = level;
    c->slots = slots;
    c->scale = scale;
    c->limbs = limbs;
    return c;
}

// The tail of a stacked product of `members` HMults at a's level: the refusals
// mul raises, the three counters, d01 / d2, the caller's tensor(d01, d2) launch
// into them (with its own count_bytes terms), then ModUp, the key switch and
// the rescale into a stack of `members` one level down.
template <class Tensor>
CtPtr Engine::product_tail(const Ciphertext &a, int members, Tensor &&tensor) {
    auto &I = *impl;
    if (a.level >= I.P.L) throw std::runtime_error("mul: no levels left");
    if (!I.ks->relin) throw std::runtime_error("mul: no relinearisation key");
    ctr.hmult += members;
    ctr.keyswitch += members;
    ctr.rescale += members;
    const size_t nn = n(), ell = a.limbs;
    auto d01m = I.alloc((size_t)members * 2 * ell * nn * 8), d2m = I.alloc((size_t)members * ell * nn * 8);
    u64 *d01 = static_cast<u64 *>(d01m->p), *d2 = static_cast<u64 *>(d2m->p);
    tensor(d01, d2);
    const bool fuse = I.ks_fuse(members);
    auto extm = I.modup(d2, ell, members, ell * nn, fuse);
    auto r = new_ct(a.level + 1, a.slots, I.P.delta[a.level + 1], ell - 1, members);
    I.mul_tail(static_cast<u64 *>(extm->p), d01, d2, ell, members, r->data, fuse);
    return r;
}

// ================================================================ keys ====
namespace {
std::vector<int64_t> sample_coeffs(const host::Entropy &ent, u64 tag, size_t n, bool ternary) {
    host::Prng g(ent, tag);
    std::vector<int64_t> v(n);
    for (size_t k = 0; k < n; ++k) v[k] = ternary ? host::sample_ternary(g) : host::sample_cbd(g);
    return v;
}
}  // namespace

void Engine::keygen() {
    auto &I = *impl;
    const size_t n = I.n(), nall = I.P.nall(), nq = I.P.nq();
    // secret over every prime
    auto s = sample_coeffs(I.ent, host::tags::secret, n, true);
    auto coef = I.alloc(n * 8);
    HIP_OK(hipMemcpyAsync(coef->p, s.data(), n * 8, hipMemcpyHostToDevice, I.st));
    I.ks->s_ntt = I.alloc(nall * n * 8);
    u64 *S = static_cast<u64 *>(I.ks->s_ntt->p);
    dev::ew_signed_to_rns(S, static_cast<int64_t *>(coef->p), (int)nall, nullptr, I.mods, I.P.logN, I.st);
    dev::ntt_forward(S, (int)nall, 1, 0, nullptr, I.T, I.st);
    // public key
    std::vector<u64> a(nq * n);
    {
        host::Prng g(I.ent, host::tags::pk_a, true);
        for (size_t l = 0; l < nq; ++l)
            for (size_t k = 0; k < n; ++k) a[l * n + k] = host::sample_uniform_mod(g, I.P.primes[l]);
    }
    auto e = sample_coeffs(I.ent, host::tags::pk_e, n, false);
    I.ks->pk = I.alloc(2 * nq * n * 8);
    u64 *pk = static_cast<u64 *>(I.ks->pk->p);
    HIP_OK(hipMemcpyAsync(pk + nq * n, a.data(), nq * n * 8, hipMemcpyHostToDevice, I.st));
    auto ec = I.alloc(n * 8);
    HIP_OK(hipMemcpyAsync(ec->p, e.data(), n * 8, hipMemcpyHostToDevice, I.st));
    auto tmp = I.alloc(nq * n * 8);
    u64 *t = static_cast<u64 *>(tmp->p);
    dev::ew_signed_to_rns(pk, static_cast<int64_t *>(ec->p), (int)nq, nullptr, I.mods, I.P.logN, I.st);
    dev::ntt_forward(pk, (int)nq, 1, 0, nullptr, I.T, I.st);
    dev::ew_mul_plain(t, pk + nq * n, S, (int)nq, 1, dev::Seg{0, 0, 0}, I.mods, I.P.logN, I.st);
    dev::ew_sub(pk, pk, t, (int)nq, 1, dev::Seg{0, 0, 0}, I.mods, I.P.logN, I.st);
    HIP_OK(hipStreamSynchronize(I.st));
    // relinearisation key: s' = s^2
    auto s2 = I.alloc(nq * n * 8);
    dev::ew_mul_plain(static_cast<u64 *>(s2->p), S, S, (int)nq, 1, dev::Seg{0, 0, 0}, I.mods, I.P.logN, I.st);
    I.ks->relin = I.alloc((size_t)I.key_digits * 2 * nall * n * 8);
    // (key material generated by the shared helper below)
    extern void gen_switch_key_impl(Engine::Impl &I, const u64 *sp, u64 kid, u64 *out);
    gen_switch_key_impl(I, static_cast<u64 *>(s2->p), 0, static_cast<u64 *>(I.ks->relin->p));
    HIP_OK(hipStreamSynchronize(I.st));
}

// ---- public stream v1: the switching keys' uniform halves from a public seed
namespace {
// enqueue the expansion of a_digit of key `kid` into out [nall][n]
void expand_public(Engine::Impl &I, const PublicSeed &seed, u64 kid, int digit, u64 *out) {
    if (!I.pub_err) {
        I.pub_err = I.alloc(sizeof(uint32_t));
        HIP_OK(hipMemsetAsync(I.pub_err->p, 0, sizeof(uint32_t), I.st));
    }
    uint32_t key[8];
    host::public_seed_key(seed.data(), key);
    dev::expand_uniform(out, key, (uint32_t)kid, digit, (int)I.P.nall(), I.mods, I.P.logN,
                        static_cast<uint32_t *>(I.pub_err->p), I.st);
}
// after the expansions of key `kid`: drains the stream and throws if a
// coefficient exhausted its attempts (the host stream names the digit)
void check_expansion(Engine::Impl &I, const PublicSeed &seed, u64 kid) {
    if (!I.pub_err) return;
    uint32_t err = 0;
    HIP_OK(hipMemcpyAsync(&err, I.pub_err->p, sizeof err, hipMemcpyDeviceToHost, I.st));
    HIP_OK(hipStreamSynchronize(I.st));
    if (!err) return;
    HIP_OK(hipMemsetAsync(I.pub_err->p, 0, sizeof(uint32_t), I.st));
    std::vector<u64> a(I.P.nall() * I.n());
    int bad = -1;
    for (int j = 0; j < I.key_digits && bad < 0; ++j)
        if (!host::public_stream_v1(seed.data(), kid, j, I.P.primes.data(), 0, I.P.nall(), I.n(), a.data())) bad = j;
    throw std::runtime_error("public stream v1: a coefficient of key " + std::to_string(kid) +
                             (bad >= 0 ? ", digit " + std::to_string(bad) : std::string()) +
                             " found no candidate below its prime in " + std::to_string(host::kPublicAttempts) +
                             " attempts");
}
}  // namespace

void gen_switch_key_impl(Engine::Impl &I, const u64 *sp, u64 kid, u64 *out) {
    const size_t n = I.n(), nall = I.P.nall(), nq = I.P.nq();
    const u64 *S = static_cast<const u64 *>(I.ks->s_ntt->p);
    const int digits = I.key_digits;
    // P mod q_i
    std::vector<int64_t> Pmod(nq);
    for (size_t i = 0; i < nq; ++i) {
        host::Modulus mi(I.P.primes[i]);
        u64 acc = 1 % mi.q;
        for (int k = 0; k < I.P.K; ++k) acc = host::mulmod(acc, I.P.primes[nq + k] % mi.q, mi);
        Pmod[i] = (int64_t)acc;
    }
    // sample every digit's (a_j, e_j) on host threads, then combine on the GPU;
    // under a public seed a_j is expanded on the device instead (public stream v1)
    const bool seeded = I.ks->has_pub_seed;
    const PublicSeed pub = I.ks->pub_seed;
    std::vector<std::vector<u64>> A(digits);
    std::vector<std::vector<int64_t>> E(digits);
    {
        std::vector<std::thread> th;
        for (int j = 0; j < digits; ++j)
            th.emplace_back([&, j]() {
                if (!seeded) {
                    host::Prng ga(I.ent, host::tags::swk_a(kid, j), true);
                    A[j].resize(nall * n);
                    for (size_t l = 0; l < nall; ++l)
                        for (size_t k = 0; k < n; ++k) A[j][l * n + k] = host::sample_uniform_mod(ga, I.P.primes[l]);
                }
                host::Prng ge(I.ent, host::tags::swk_e(kid, j));
                E[j].resize(n);
                for (size_t k = 0; k < n; ++k) E[j][k] = host::sample_cbd(ge);
            });
        for (auto &t : th) t.join();
    }
    auto ec = I.alloc(n * 8);
    auto tmpm = I.alloc(nall * n * 8);
    u64 *tmp = static_cast<u64 *>(tmpm->p);
    for (int j = 0; j < digits; ++j) {
        u64 *bj = out + ((size_t)j * 2 + 0) * nall * n;
        u64 *aj = out + ((size_t)j * 2 + 1) * nall * n;
        if (seeded)
            expand_public(I, pub, kid, j, aj);
        else
            HIP_OK(hipMemcpyAsync(aj, A[j].data(), nall * n * 8, hipMemcpyHostToDevice, I.st));
        HIP_OK(hipMemcpyAsync(ec->p, E[j].data(), n * 8, hipMemcpyHostToDevice, I.st));
        dev::ew_signed_to_rns(bj, static_cast<int64_t *>(ec->p), (int)nall, nullptr, I.mods, I.P.logN, I.st);
        dev::ntt_forward(bj, (int)nall, 1, 0, nullptr, I.T, I.st);
        dev::ew_mul_plain(tmp, aj, S, (int)nall, 1, dev::Seg{0, 0, 0}, I.mods, I.P.logN, I.st);
        dev::ew_sub(bj, bj, tmp, (int)nall, 1, dev::Seg{0, 0, 0}, I.mods, I.P.logN, I.st);
        const size_t lo = (size_t)j * I.P.alpha, hi = std::min(nq, (size_t)(j + 1) * I.P.alpha);
        dev::LimbConsts W{};  // + P s' over the digit's primes, one launch
        for (size_t i = lo; i < hi; ++i) W.w[i - lo] = (u64)Pmod[i];
        dev::ew_add_scaled(bj + lo * n, sp + lo * n, W, (int)(hi - lo), dev::Seg{0, 0, 0}, I.mods + lo, I.P.logN, I.st);
        HIP_OK(hipStreamSynchronize(I.st));  // host buffers A[j], E[j] go out of scope after the loop
    }
    if (seeded) {
        check_expansion(I, pub, kid);
        I.ks->seeded[kid] = pub;
    } else {
        I.ks->seeded.erase(kid);
    }
}

void Engine::gen_rotation_keys(const std::vector<int> &rot) {
    std::vector<u64> gs;
    for (int k : rot) gs.push_back(host::galois_for_rotation(impl->P.logN, k));
    gen_galois_keys(gs);
}

void Engine::gen_galois_keys(const std::vector<u64> &gs) {
    auto &I = *impl;
    const size_t n = I.n(), nq = I.P.nq(), nall = I.P.nall();
    if (!I.ks->s_ntt) throw std::runtime_error("gen_rotation_keys: no secret key (call keygen)");
    auto sp = I.alloc(nq * n * 8);
    for (u64 g : gs) {
        if (g == 1 || I.ks->rotkeys.count(g)) continue;
        dev::ew_permute(static_cast<u64 *>(sp->p), static_cast<const u64 *>(I.ks->s_ntt->p), I.perm(g), (int)nq, 1, dev::Seg{0, 0, 0},
                        I.P.logN, I.st);
        auto key = I.alloc((size_t)I.key_digits * 2 * nall * n * 8);
        gen_switch_key_impl(I, static_cast<u64 *>(sp->p), g, static_cast<u64 *>(key->p));
        I.ks->rotkeys[g] = key;
    }
    HIP_OK(hipStreamSynchronize(I.st));
}

// Keys are replaced in the KeySet shared with forked engines, from pooled
// blocks: drain every stream of the device first (this engine's, its forks',
// anyone's), so no kernel still reads the key being replaced and no pending
// work still owns the block the pool hands out for the new one.
namespace {
void drain_before_key_load() { HIP_OK(hipDeviceSynchronize()); }
}  // namespace

void Engine::load_secret(const u64 *s) {
    auto &I = *impl;
    drain_before_key_load();
    const size_t bytes = I.P.nall() * I.n() * 8;
    I.ks->s_ntt = I.alloc(bytes);
    HIP_OK(hipMemcpy(I.ks->s_ntt->p, s, bytes, hipMemcpyHostToDevice));
}
void Engine::load_public(const u64 *pk) {
    auto &I = *impl;
    drain_before_key_load();
    const size_t bytes = 2 * I.P.nq() * I.n() * 8;
    I.ks->pk = I.alloc(bytes);
    HIP_OK(hipMemcpy(I.ks->pk->p, pk, bytes, hipMemcpyHostToDevice));
}
void Engine::load_relin(const u64 *key) {
    auto &I = *impl;
    drain_before_key_load();
    const size_t bytes = (size_t)I.key_digits * 2 * I.P.nall() * I.n() * 8;
    I.ks->relin = I.alloc(bytes);
    HIP_OK(hipMemcpy(I.ks->relin->p, key, bytes, hipMemcpyHostToDevice));
    I.ks->seeded.erase(0);
}
void Engine::load_rotation(long k, const u64 *key) {
    auto &I = *impl;
    drain_before_key_load();
    const size_t bytes = (size_t)I.key_digits * 2 * I.P.nall() * I.n() * 8;
    const u64 g = host::galois_for_rotation(I.P.logN, k);
    auto m = I.alloc(bytes);
    HIP_OK(hipMemcpy(m->p, key, bytes, hipMemcpyHostToDevice));
    I.ks->rotkeys[g] = m;
    I.ks->seeded.erase(g);
}
void Engine::load_galois(u64 g, const u64 *key) {
    auto &I = *impl;
    drain_before_key_load();
    const size_t bytes = (size_t)I.key_digits * 2 * I.P.nall() * I.n() * 8;
    auto m = I.alloc(bytes);
    HIP_OK(hipMemcpy(m->p, key, bytes, hipMemcpyHostToDevice));
    I.ks->rotkeys[g] = m;
    I.ks->seeded.erase(g);
}
// a seeded key: the b halves [digits][nall][n] from the host, the a halves
// expanded on the device
namespace {
std::shared_ptr<DevMem> load_seeded_key(Engine::Impl &I, const PublicSeed &seed, u64 kid, const u64 *b) {
    drain_before_key_load();
    const size_t half = I.P.nall() * I.n();
    auto m = I.alloc((size_t)I.key_digits * 2 * half * 8);
    u64 *key = static_cast<u64 *>(m->p);
    HIP_OK(hipMemcpy2D(key, 2 * half * 8, b, half * 8, half * 8, (size_t)I.key_digits, hipMemcpyHostToDevice));
    for (int j = 0; j < I.key_digits; ++j) expand_public(I, seed, kid, j, key + ((size_t)j * 2 + 1) * half);
    check_expansion(I, seed, kid);
    return m;
}
}  // namespace
void Engine::load_relin_seeded(const uint8_t seed[32], const u64 *b) {
    PublicSeed s;
    std::memcpy(s.data(), seed, 32);
    impl->ks->relin = load_seeded_key(*impl, s, 0, b);
    impl->ks->seeded[0] = s;
}
void Engine::load_galois_seeded(const uint8_t seed[32], u64 g, const u64 *b) {
    PublicSeed s;
    std::memcpy(s.data(), seed, 32);
    impl->ks->rotkeys[g] = load_seeded_key(*impl, s, g, b);
    impl->ks->seeded[g] = s;
}
void Engine::set_public_seed(const uint8_t seed[32]) {
    std::memcpy(impl->ks->pub_seed.data(), seed, 32);
    impl->ks->has_pub_seed = true;
}
bool Engine::get_public_seed(uint8_t seed[32]) const {
    if (!impl->ks->has_pub_seed) return false;
    std::memcpy(seed, impl->ks->pub_seed.data(), 32);
    return true;
}
int Engine::key_seeded(u64 kid, uint8_t *seed) const {
    const auto &K = *impl->ks;
    if (kid == 0 ? !K.relin : !K.rotkeys.count(kid)) return -1;
    auto it = K.seeded.find(kid);
    if (it == K.seeded.end()) return 0;
    if (seed) std::memcpy(seed, it->second.data(), 32);
    return 1;
}
void Engine::public_poly(const uint8_t seed[32], u64 kid, int digit, u64 *out) {
    auto &I = *impl;
    if (digit < 0 || digit >= I.key_digits) throw std::invalid_argument("public_poly: digit out of range");
    if (kid >> 32) throw std::invalid_argument("public_poly: key id beyond 32 bits");
    PublicSeed s;
    std::memcpy(s.data(), seed, 32);
    const size_t words = I.P.nall() * I.n();
    auto m = I.alloc(words * 8);
    expand_public(I, s, kid, digit, static_cast<u64 *>(m->p));
    check_expansion(I, s, kid);
    HIP_OK(hipMemcpy(out, m->p, words * 8, hipMemcpyDeviceToHost));
}
bool Engine::has_galois_key(u64 g) const { return impl->ks->rotkeys.count(g) > 0; }
bool Engine::has_rotation_key(long k) const {
    return impl->ks->rotkeys.count(host::galois_for_rotation(impl->P.logN, k)) > 0;
}
int Engine::key_digits() const { return impl->key_digits; }
size_t Engine::switch_key_words() const { return (size_t)impl->key_digits * 2 * impl->P.nall() * impl->P.n; }
bool Engine::has_secret() const { return (bool)impl->ks->s_ntt; }
bool Engine::has_public() const { return (bool)impl->ks->pk; }
bool Engine::has_relin() const { return (bool)impl->ks->relin; }
namespace {
void export_key(Engine::Impl &I, const std::shared_ptr<DevMem> &m, size_t words, u64 *out, const char *what) {
    if (!m) throw std::invalid_argument(std::string("export: no ") + what);
    HIP_OK(hipStreamSynchronize(I.st));
    HIP_OK(hipMemcpy(out, m->p, words * 8, hipMemcpyDeviceToHost));
}
}  // namespace
void Engine::export_secret(u64 *out) { export_key(*impl, impl->ks->s_ntt, impl->P.nall() * n(), out, "secret key"); }
void Engine::export_public(u64 *out) { export_key(*impl, impl->ks->pk, 2 * impl->P.nq() * n(), out, "public key"); }
void Engine::export_relin(u64 *out) { export_key(*impl, impl->ks->relin, switch_key_words(), out, "relinearisation key"); }
std::vector<u64> Engine::galois_elements() const {
    std::vector<u64> gs;
    for (auto &kv : impl->ks->rotkeys) gs.push_back(kv.first);
    return gs;
}
void Engine::export_galois(u64 g, u64 *out) {
    auto it = impl->ks->rotkeys.find(g);
    if (it == impl->ks->rotkeys.end()) throw std::invalid_argument("export: no key for galois element " + std::to_string(g));
    export_key(*impl, it->second, switch_key_words(), out, "galois key");
}
namespace {
// the b halves [digits][nall][n] of a switching key
void export_key_b(Engine::Impl &I, const std::shared_ptr<DevMem> &m, u64 *out, const char *what) {
    if (!m) throw std::invalid_argument(std::string("export: no ") + what);
    const size_t half = I.P.nall() * I.n();
    HIP_OK(hipStreamSynchronize(I.st));
    HIP_OK(hipMemcpy2D(out, half * 8, m->p, 2 * half * 8, half * 8, (size_t)I.key_digits, hipMemcpyDeviceToHost));
}
}  // namespace
void Engine::export_relin_b(u64 *out) { export_key_b(*impl, impl->ks->relin, out, "relinearisation key"); }
void Engine::export_galois_b(u64 g, u64 *out) {
    auto it = impl->ks->rotkeys.find(g);
    if (it == impl->ks->rotkeys.end()) throw std::invalid_argument("export: no key for galois element " + std::to_string(g));
    export_key_b(*impl, it->second, out, "galois key");
}
size_t Engine::key_bytes() const {
    size_t b = impl->ks->relin ? impl->ks->relin->bytes : 0;
    for (auto &kv : impl->ks->rotkeys) b += kv.second->bytes;
    return b;
}

// ==================================================== encode / encrypt ====
PtPtr Engine::encode(const std::vector<double> &v, int slots, int level) {
    return encode_scaled(v, slots, level, impl->P.delta[level]);
}
PtPtr Engine::encode_scaled(const std::vector<double> &v, int slots, int level, double scale) {
    auto &I = *impl;
    const u64 t0 = now_ns();
    const size_t n = I.n(), ell = I.P.limbs_at(level);
    auto coef = host::encode_coeffs(v, n, slots, scale);
    auto cm = I.alloc(n * 8);
    HIP_OK(hipMemcpyAsync(cm->p, coef.data(), n * 8, hipMemcpyHostToDevice, I.st));
    auto pt = std::make_shared<Plaintext>();
    pt->mem = I.alloc(ell * n * 8);
    pt->data = static_cast<u64 *>(pt->mem->p);
    pt->level = level;
    pt->slots = slots;
    pt->scale = scale;
    pt->limbs = ell;
    dev::ew_signed_to_rns(pt->data, static_cast<int64_t *>(cm->p), (int)ell, nullptr, I.mods, I.P.logN, I.st);
    dev::ntt_forward(pt->data, (int)ell, 1, 0, nullptr, I.T, I.st);
    HIP_OK(hipStreamSynchronize(I.st));  // `coef` (pageable host) must outlive the copy
    host_stats().encode_ns += now_ns() - t0;
    host_stats().encodes++;
    return pt;
}

std::vector<PtPtr> Engine::encode_masks(const std::vector<MaskSpec> &specs, int num_slots, int N) {
    auto &I = *impl;
    const int B = (int)specs.size();
    if (B == 0) return {};
    if (num_slots <= 0 || (num_slots & (num_slots - 1)) || (size_t)num_slots > I.n() / 2 || N <= 0)
        throw std::invalid_argument("encode_masks: slots must be a power of two <= n/2");
    const u64 t0 = now_ns();
    I.enc_tables();
    std::vector<int> ord(B);
    for (int i = 0; i < B; ++i) ord[i] = i;
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return specs[a].level < specs[b].level; });
    std::vector<int> spec(3 * B), levels(B);
    std::vector<double> scales(B);
    for (int j = 0; j < B; ++j) {
        const MaskSpec &m = specs[ord[j]];
        if (m.level < 0 || m.level > I.P.L) throw std::invalid_argument("encode_masks: level out of range");
        spec[3 * j] = m.kind;
        spec[3 * j + 1] = m.k;
        spec[3 * j + 2] = m.r;
        levels[j] = m.level;
        scales[j] = I.P.delta[m.level];
    }
    auto vm = I.alloc((size_t)B * num_slots * sizeof(double2));
    double2 *v = static_cast<double2 *>(vm->p);
    auto sm = I.alloc(spec.size() * 4);
    HIP_OK(hipMemcpyAsync(sm->p, spec.data(), spec.size() * 4, hipMemcpyHostToDevice, I.st));
    dev::mask_slots(v, B, num_slots, N, static_cast<const int *>(sm->p), I.st);
    auto sorted = I.encode_sorted(v, B, num_slots, levels, scales);  // synchronises: `spec` outlives its copy
    std::vector<PtPtr> out(B);
    for (int j = 0; j < B; ++j) out[ord[j]] = sorted[j];
    host_stats().encode_ns += now_ns() - t0;
    host_stats().encodes += B;
    return out;
}

int Engine::select_cap(int N, int num_slots) {
    if (N < 1 || (N & (N - 1)) || num_slots < N || num_slots % N)
        throw std::invalid_argument("select layout: N must be a power of two and num_slots a multiple of it");
    const int parts = num_slots / N;
    if ((parts & (parts - 1)) || parts > N)
        throw std::invalid_argument("select layout: num_slots / N must be a power of two <= N");
    return parts >= 2 ? parts - 1 : 1;
}

std::array<PtPtr, 2> Engine::encode_select(const std::vector<int> &targets, int member, int num_slots, int N,
                                           int level_c, int level_k) {
    auto &I = *impl;
    const int cap = select_cap(N, num_slots);
    if ((size_t)num_slots > I.n() / 2) throw std::invalid_argument("encode_select: slots must be a power of two <= n/2");
    const int k = (int)targets.size();
    if (k < 1 || k > N) throw std::invalid_argument("encode_select: the target count must lie in 1..N");
    if (member < 0 || (long long)member * cap >= k) throw std::invalid_argument("encode_select: no such member");
    for (int lv : {level_c, level_k})
        if (lv < 0 || lv > I.P.L) throw std::invalid_argument("encode_select: level out of range");
    const int first = member * cap, cnt = std::min(cap, k - first);
    for (int q = 0; q < cnt; ++q)
        if (targets[first + q] < 0 || targets[first + q] >= N)
            throw std::invalid_argument("encode_select: target " + std::to_string(first + q) + " is outside [0, N)");
    const u64 t0 = now_ns();
    I.enc_tables();
    // encode_sorted takes its members in level order
    const int ic = level_c <= level_k ? 0 : 1, ik = 1 - ic;
    std::vector<int> levels(2);
    std::vector<double> scales(2);
    levels[ic] = level_c;
    levels[ik] = level_k;
    scales[ic] = I.P.delta[level_c];
    scales[ik] = I.P.delta[level_k];
    auto vm = I.alloc((size_t)2 * num_slots * sizeof(double2));
    double2 *v = static_cast<double2 *>(vm->p);
    auto tm = I.alloc((size_t)cnt * 4);
    HIP_OK(hipMemcpyAsync(tm->p, targets.data() + first, (size_t)cnt * 4, hipMemcpyHostToDevice, I.st));
    dev::select_slots(v + (size_t)ic * num_slots, v + (size_t)ik * num_slots, num_slots, N,
                      static_cast<const int *>(tm->p), cnt, first % num_slots, I.st);
    auto sorted = I.encode_sorted(v, 2, num_slots, levels, scales);  // synchronises: `targets` outlives its copy
    host_stats().encode_ns += now_ns() - t0;
    host_stats().encodes += 2;
    return {sorted[ic], sorted[ik]};
}

std::vector<double> Engine::tiebreak_offsets(int N, int num_slots, int batch, double eps) {
    select_cap(N, num_slots);  // validates the shape
    const int parts = num_slots / N;
    if (batch < 0 || (long long)batch * parts >= N)
        throw std::invalid_argument("tiebreak offsets: batch " + std::to_string(batch) + " is outside [0, N / (num_slots / N))");
    if (!(eps >= 0.0 && eps < 0.5)) throw std::invalid_argument("tiebreak offsets: eps must lie in [0, 0.5)");
    std::vector<double> v((size_t)num_slots);
    for (int s = 0; s < num_slots; ++s) {
        const long long t = (long long)batch * parts + s / N;
        v[(size_t)s] = (t == 0 || s % N + t >= N) ? eps : -eps;
    }
    return v;
}

std::vector<PtPtr> Engine::encode_tiebreak(const std::vector<int> &batches, int num_slots, int N, double eps, int level) {
    auto &I = *impl;
    const int B = (int)batches.size();
    if (B == 0) return {};
    select_cap(N, num_slots);  // validates the shape
    const int parts = num_slots / N;
    if ((size_t)num_slots > I.n() / 2) throw std::invalid_argument("encode_tiebreak: slots must be a power of two <= n/2");
    if (!(eps >= 0.0 && eps < 0.5)) throw std::invalid_argument("encode_tiebreak: eps must lie in [0, 0.5)");
    if (level < 0 || level > I.P.L) throw std::invalid_argument("encode_tiebreak: level out of range");
    for (int b : batches)
        if (b < 0 || (long long)b * parts >= N)
            throw std::invalid_argument("encode_tiebreak: batch " + std::to_string(b) + " is outside [0, N / (num_slots / N))");
    const u64 t0 = now_ns();
    I.enc_tables();
    const std::vector<int> levels((size_t)B, level);
    const std::vector<double> scales((size_t)B, I.P.delta[level]);
    auto vm = I.alloc((size_t)B * num_slots * sizeof(double2));
    auto bm = I.alloc((size_t)B * 4);
    HIP_OK(hipMemcpyAsync(bm->p, batches.data(), (size_t)B * 4, hipMemcpyHostToDevice, I.st));
    dev::tiebreak_slots(static_cast<double2 *>(vm->p), B, num_slots, N, static_cast<const int *>(bm->p), eps, I.st);
    auto out = I.encode_sorted(static_cast<double2 *>(vm->p), B, num_slots, levels, scales);  // synchronises: `batches` outlives its copy
    host_stats().encode_ns += now_ns() - t0;
    host_stats().encodes += B;
    return out;
}

std::vector<PtPtr> Engine::encode_device(const std::vector<std::vector<double>> &vs, int slots,
                                         const std::vector<int> &levels) {
    auto &I = *impl;
    const int B = (int)vs.size();
    if (B == 0) return {};
    if ((int)levels.size() != B) throw std::invalid_argument("encode_device: one level per vector");
    if (slots <= 0 || (slots & (slots - 1)) || (size_t)slots > I.n() / 2)
        throw std::invalid_argument("encode: slots must be a power of two <= n/2");
    I.enc_tables();
    std::vector<int> ord(B);
    for (int i = 0; i < B; ++i) ord[i] = i;
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return levels[a] < levels[b]; });
    std::vector<double> h((size_t)2 * B * slots, 0.0), scales(B);
    std::vector<int> lv(B);
    for (int j = 0; j < B; ++j) {
        const auto &x = vs[ord[j]];
        for (size_t i = 0; i < x.size() && i < (size_t)slots; ++i) h[2 * ((size_t)j * slots + i)] = x[i];
        lv[j] = levels[ord[j]];
        if (lv[j] < 0 || lv[j] > I.P.L) throw std::invalid_argument("encode_device: level out of range");
        scales[j] = I.P.delta[lv[j]];
    }
    auto vm = I.alloc(h.size() * 8);
    HIP_OK(hipMemcpyAsync(vm->p, h.data(), h.size() * 8, hipMemcpyHostToDevice, I.st));
    auto sorted = I.encode_sorted(static_cast<double2 *>(vm->p), B, slots, lv, scales);
    std::vector<PtPtr> out(B);
    for (int j = 0; j < B; ++j) out[ord[j]] = sorted[j];
    return out;
}

void Engine::host_stats_get(double out[4]) {
    out[0] = (double)host_stats().encodes.load();
    out[1] = (double)host_stats().encode_ns.load() * 1e-9;
    out[2] = (double)host_stats().mallocs.load();
    out[3] = (double)host_stats().malloc_ns.load() * 1e-9;
}
void Engine::host_stats_reset() {
    host_stats().encodes = 0;
    host_stats().encode_ns = 0;
    host_stats().mallocs = 0;
    host_stats().malloc_ns = 0;
}

PtPtr Engine::encode_complex(const std::vector<std::complex<double>> &v, int slots, int level, double scale) {
    auto &I = *impl;
    const size_t n = I.n(), ell = I.P.limbs_at(level);
    auto coef = host::encode_coeffs_complex(v, n, slots, scale);
    auto cm = I.alloc(n * 8);
    HIP_OK(hipMemcpyAsync(cm->p, coef.data(), n * 8, hipMemcpyHostToDevice, I.st));
    auto pt = std::make_shared<Plaintext>();
    pt->mem = I.alloc(ell * n * 8);
    pt->data = static_cast<u64 *>(pt->mem->p);
    pt->level = level;
    pt->slots = slots;
    pt->scale = scale;
    pt->limbs = ell;
    dev::ew_signed_to_rns(pt->data, static_cast<int64_t *>(cm->p), (int)ell, nullptr, I.mods, I.P.logN, I.st);
    dev::ntt_forward(pt->data, (int)ell, 1, 0, nullptr, I.T, I.st);
    HIP_OK(hipStreamSynchronize(I.st));  // `coef` (pageable host) must outlive the copy
    return pt;
}

PtPtr Engine::encode_complex_ext(const std::vector<std::complex<double>> &v, int slots, int level, double scale) {
    auto &I = *impl;
    const size_t n = I.n(), ell = I.P.limbs_at(level), W = ell + (size_t)I.P.K;
    auto coef = host::encode_coeffs_complex(v, n, slots, scale);
    auto cm = I.alloc(n * 8);
    HIP_OK(hipMemcpyAsync(cm->p, coef.data(), n * 8, hipMemcpyHostToDevice, I.st));
    auto pt = std::make_shared<Plaintext>();
    pt->mem = I.alloc(W * n * 8);
    pt->data = static_cast<u64 *>(pt->mem->p);
    pt->level = level;
    pt->slots = slots;
    pt->scale = scale;
    pt->limbs = W;
    dev::ew_signed_to_rns(pt->data, static_cast<int64_t *>(cm->p), (int)W, I.ext(ell), I.mods, I.P.logN, I.st);
    dev::ntt_forward(pt->data, (int)W, 1, 0, I.ext(ell), I.T, I.st);
    HIP_OK(hipStreamSynchronize(I.st));  // `coef` (pageable host) must outlive the copy
    return pt;
}

CtPtr Engine::encrypt_pt(const Plaintext &pt) {
    auto &I = *impl;
    if (!I.ks->pk) throw std::runtime_error("encrypt: no public key");
    const size_t n = I.n(), nq = I.P.nq(), ell = pt.limbs;
    const u64 c = (*I.enc_counter)++;
    std::vector<int64_t> smp(3 * n);
    {
        auto v = sample_coeffs(I.ent, host::tags::enc_v(c), n, true);
        auto e0 = sample_coeffs(I.ent, host::tags::enc_e0(c), n, false);
        auto e1 = sample_coeffs(I.ent, host::tags::enc_e1(c), n, false);
        std::copy(v.begin(), v.end(), smp.begin());
        std::copy(e0.begin(), e0.end(), smp.begin() + n);
        std::copy(e1.begin(), e1.end(), smp.begin() + 2 * n);
    }
    auto sm = I.alloc(3 * n * 8);
    HIP_OK(hipMemcpyAsync(sm->p, smp.data(), 3 * n * 8, hipMemcpyHostToDevice, I.st));
    auto rm = I.alloc(3 * ell * n * 8);
    u64 *r = static_cast<u64 *>(rm->p);
    for (int i = 0; i < 3; ++i)
        dev::ew_signed_to_rns(r + i * ell * n, static_cast<int64_t *>(sm->p) + i * n, (int)ell, nullptr, I.mods,
                              I.P.logN, I.st);
    dev::ntt_forward(r, (int)ell, 3, ell * n, nullptr, I.T, I.st);
    auto ct = new_ct(pt.level, pt.slots, pt.scale, ell);
    const u64 *pk = static_cast<const u64 *>(I.ks->pk->p);
    u64 *c0 = ct->data, *c1 = ct->data + ell * n;
    dev::ew_mul_plain(c0, r, pk, (int)ell, 1, dev::Seg{0, 0, 0}, I.mods, I.P.logN, I.st);
    dev::ew_add(c0, c0, r + ell * n, (int)ell, 1, dev::Seg{0, 0, 0}, I.mods, I.P.logN, I.st);
    dev::ew_add(c0, c0, pt.data, (int)ell, 1, dev::Seg{0, 0, 0}, I.mods, I.P.logN, I.st);
    dev::ew_mul_plain(c1, r, pk + nq * n, (int)ell, 1, dev::Seg{0, 0, 0}, I.mods, I.P.logN, I.st);
    dev::ew_add(c1, c1, r + 2 * ell * n, (int)ell, 1, dev::Seg{0, 0, 0}, I.mods, I.P.logN, I.st);
    HIP_OK(hipStreamSynchronize(I.st));
    return ct;
}

CtPtr Engine::encrypt(const std::vector<double> &v, int slots, int level) {
    return encrypt_pt(*encode(v, slots, level));
}

// FLEXIBLEAUTOEXT-style fresh encryption (oracle: Context::encrypt_ext): encode
// at Delta_1 on the level-0 basis, times q_L, encrypt, rescale by q_L -- the
// encryption noise shrinks by q_L; result at level 1, scale Delta_1
CtPtr Engine::encrypt_ext(const std::vector<double> &v, int slots) {
    auto &I = *impl;
    if (I.P.L < 1) throw std::runtime_error("encrypt_ext: needs one extra level");
    PtPtr pt = encode_scaled(v, slots, 0, I.P.delta[1]);
    const u64 qL = I.P.primes[I.P.nq() - 1];
    dev::ew_mul_scalar(pt->data, pt->data, (int64_t)qL, (int)pt->limbs, 1, dev::Seg{0, 0, 0}, I.mods, I.P.logN,
                       I.st);
    pt->scale = I.P.delta[1] * (double)qL;
    CtPtr r = rescale(*encrypt_pt(*pt));
    r->scale = I.P.delta[1];
    return r;
}

std::vector<double> Engine::decrypt(const Ciphertext &ct) {
    auto &I = *impl;
    if (ct.batch != 1) throw std::invalid_argument("decrypt: one ciphertext at a time (use member())");
    if (!I.ks->s_ntt) throw std::runtime_error("decrypt: no secret key");
    const size_t n = I.n();
    const int L2 = ct.limbs >= 2 ? 2 : 1;  // m = c0 + c1 s on the first one or two limbs
    auto mm = I.alloc(L2 * n * 8);
    u64 *m = static_cast<u64 *>(mm->p);
    dev::ew_mul_plain(m, ct.data + ct.limbs * n, static_cast<const u64 *>(I.ks->s_ntt->p), L2, 1, dev::Seg{0, 0, 0}, I.mods, I.P.logN,
                      I.st);
    dev::ew_add(m, m, ct.data, L2, 1, dev::Seg{0, 0, 0}, I.mods, I.P.logN, I.st);
    dev::ntt_inverse(m, L2, 1, 0, nullptr, I.T, I.st);
    std::vector<u64> h(L2 * n);
    HIP_OK(hipMemcpyAsync(h.data(), m, L2 * n * 8, hipMemcpyDeviceToHost, I.st));
    HIP_OK(hipStreamSynchronize(I.st));
    return host::decode_coeffs(h.data(), L2 == 2 ? h.data() + n : nullptr, n, I.P.primes[0],
                               L2 == 2 ? I.P.primes[1] : 0, ct.slots, ct.scale);
}

CtPtr Engine::upload(const u64 *h, size_t limbs, int level, int slots, double scale) {
    auto ct = new_ct(level, slots, scale, limbs);
    HIP_OK(hipMemcpyAsync(ct->data, h, 2 * limbs * n() * 8, hipMemcpyHostToDevice, impl->st));
    HIP_OK(hipStreamSynchronize(impl->st));
    return ct;
}
void Engine::download(const Ciphertext &ct, u64 *h) {
    if (ct.batch != 1) throw std::invalid_argument("download: one ciphertext at a time (use member())");
    HIP_OK(hipMemcpyAsync(h, ct.data, 2 * ct.limbs * n() * 8, hipMemcpyDeviceToHost, impl->st));
    HIP_OK(hipStreamSynchronize(impl->st));
}
PtPtr Engine::upload_pt(const u64 *h, size_t limbs, int level, int slots, double scale) {
    auto pt = std::make_shared<Plaintext>();
    pt->mem = impl->alloc(limbs * n() * 8);
    pt->data = static_cast<u64 *>(pt->mem->p);
    pt->level = level;
    pt->slots = slots;
    pt->scale = scale;
    pt->limbs = limbs;
    HIP_OK(hipMemcpyAsync(pt->data, h, limbs * n() * 8, hipMemcpyHostToDevice, impl->st));
    HIP_OK(hipStreamSynchronize(impl->st));
    return pt;
}

// ================================================================= ops ====
#define LOGN impl->P.logN
#define MODS impl->mods
#define ST impl->st

// Every op below is batch-transparent: a ciphertext of `batch` members is
// [batch][2][limbs][n], i.e. 2*batch segments of stride limbs*n, and each
// kernel launch covers all of them.
namespace {
inline dev::Seg seg3(size_t o, size_t a, size_t b) { return dev::Seg{o, a, b}; }
void same_batch(const Ciphertext &a, const Ciphertext &b, const char *op) {
    if (a.batch != b.batch) throw std::invalid_argument(std::string(op) + ": batch size mismatch");
}
}  // namespace

CtPtr Engine::clone(const Ciphertext &a) {
    auto r = new_ct(a.level, a.slots, a.scale, a.limbs, a.batch);
    HIP_OK(hipMemcpyAsync(r->data, a.data, 2 * (size_t)a.batch * a.limbs * n() * 8, hipMemcpyDeviceToDevice, ST));
    return r;
}

CtPtr Engine::drop_to(const Ciphertext &a, int level) {
    if (level < a.level) throw std::invalid_argument("drop_to: cannot raise level");
    const size_t ell = impl->P.limbs_at(level), nn = n();
    auto r = new_ct(level, a.slots, a.scale, ell, a.batch);
    HIP_OK(hipMemcpy2DAsync(r->data, ell * nn * 8, a.data, a.limbs * nn * 8, ell * nn * 8, 2 * (size_t)a.batch,
                            hipMemcpyDeviceToDevice, ST));
    return r;
}

// op-level byte model (Counters::opbytes): `limb_units` limbs of n words per ciphertext, times members
void clock_phase_opbytes(const char *phase, u64 b);
void Engine::count_bytes(double limb_units, int members) {
    const u64 b = (u64)(limb_units * members * 8.0 * n());
    ctr.opbytes += b;
    if (dev::launch_clock() && dev::algo_phase()) clock_phase_opbytes(dev::algo_phase(), b);
}
double Engine::ks_units(size_t ell) const {  // 2 digits(l) (l + K): the key read of one key switch
    const auto &P = impl->P;
    return 2.0 * P.digits_at(ell) * (double)(ell + P.K);
}

void Engine::match_levels(CtPtr &a, CtPtr &b) {
    if (a->level < b->level)
        a = level_adjust(*a, b->level);
    else if (b->level < a->level)
        b = level_adjust(*b, a->level);
}

CtPtr Engine::add(const Ciphertext &a0, const Ciphertext &b0) {
    same_batch(a0, b0, "add");
    auto a = std::make_shared<Ciphertext>(a0), b = std::make_shared<Ciphertext>(b0);
    match_levels(a, b);
    const size_t ln = a->limbs * n();
    auto r = new_ct(a->level, a->slots, a->scale, a->limbs, a->batch);
    dev::ew_add(r->data, a->data, b->data, (int)a->limbs, 2 * a->batch, seg3(ln, ln, ln), MODS, LOGN, ST);
    count_bytes(6.0 * a->limbs, a->batch);
    return r;
}
CtPtr Engine::sub(const Ciphertext &a0, const Ciphertext &b0) {
    same_batch(a0, b0, "sub");
    auto a = std::make_shared<Ciphertext>(a0), b = std::make_shared<Ciphertext>(b0);
    match_levels(a, b);
    const size_t ln = a->limbs * n();
    auto r = new_ct(a->level, a->slots, a->scale, a->limbs, a->batch);
    dev::ew_sub(r->data, a->data, b->data, (int)a->limbs, 2 * a->batch, seg3(ln, ln, ln), MODS, LOGN, ST);
    count_bytes(6.0 * a->limbs, a->batch);
    return r;
}
void Engine::add_inplace(CtPtr &acc, const Ciphertext &b) {
    if (!acc) {
        acc = clone(b);
        return;
    }
    same_batch(*acc, b, "add_inplace");
    if (acc->level == b.level && acc.use_count() == 1) {
        const size_t ln = b.limbs * n();
        dev::ew_add(acc->data, acc->data, b.data, (int)b.limbs, 2 * b.batch, seg3(ln, ln, ln), MODS, LOGN, ST);
        count_bytes(6.0 * b.limbs, b.batch);
        return;
    }
    acc = add(*acc, b);
}
CtPtr Engine::negate(const Ciphertext &a) {
    const size_t ln = a.limbs * n();
    auto r = new_ct(a.level, a.slots, a.scale, a.limbs, a.batch);
    dev::ew_neg(r->data, a.data, (int)a.limbs, 2 * a.batch, seg3(ln, ln, 0), MODS, LOGN, ST);
    count_bytes(4.0 * a.limbs, a.batch);
    return r;
}
// plaintext ops touch c0 of every member: segments 0, 2, 4, ... (stride 2 limbs n)
// plaintext and constant ops change c0 only; one pass writes the whole result
// (k_c0_op: c1 copied through), so no clone precedes them
CtPtr Engine::add_plain(const Ciphertext &a, const Plaintext &p) {
    if (p.level != a.level) throw std::invalid_argument("add_plain: level mismatch");
    auto r = new_ct(a.level, a.slots, a.scale, a.limbs, a.batch);
    dev::ew_c0_op(r->data, a.data, p.data, 0, 0, 1, (int)a.limbs, a.batch, MODS, LOGN, ST);
    count_bytes(5.0 * a.limbs, a.batch);
    return r;
}
CtPtr Engine::sub_plain(const Ciphertext &a, const Plaintext &p) {
    if (p.level != a.level) throw std::invalid_argument("sub_plain: level mismatch");
    auto r = new_ct(a.level, a.slots, a.scale, a.limbs, a.batch);
    dev::ew_c0_op(r->data, a.data, p.data, 0, 0, 2, (int)a.limbs, a.batch, MODS, LOGN, ST);
    count_bytes(5.0 * a.limbs, a.batch);
    return r;
}
CtPtr Engine::plain_sub(const Plaintext &p, const Ciphertext &a) {
    if (p.level != a.level) throw std::invalid_argument("plain_sub: level mismatch");
    auto r = new_ct(a.level, a.slots, a.scale, a.limbs, a.batch);
    dev::ew_c0_op(r->data, a.data, p.data, 0, 0, 3, (int)a.limbs, a.batch, MODS, LOGN, ST);
    return r;
}
CtPtr Engine::add_const(const Ciphertext &a, double c) {
    auto r = new_ct(a.level, a.slots, a.scale, a.limbs, a.batch);
    const host::SConst K = host::const_at_scale(c, a.scale);
    dev::ew_c0_op(r->data, a.data, nullptr, K.k, K.sh, 0, (int)a.limbs, a.batch, MODS, LOGN, ST);
    count_bytes(4.0 * a.limbs, a.batch);
    return r;
}
// a + c with a exclusively owned (no other handle, no member view of its memory):
// only the c0 limbs are read and written, in place -- half the traffic of
// add_const's copy and no allocation; otherwise add_const.  Same words.
void Engine::add_const_inplace(CtPtr &a, double c) {
    if (!a) throw std::invalid_argument("add_const_inplace: empty ciphertext");
    if (a.use_count() != 1 || !a->mem || a->mem.use_count() != 1) {
        a = add_const(*a, c);
        return;
    }
    const size_t ln = a->limbs * n();
    const host::SConst K = host::const_at_scale(c, a->scale);
    dev::ew_add_scalar(a->data, a->data, K.k, (int)a->limbs, a->batch, seg3(2 * ln, 2 * ln, 0), MODS, LOGN, ST, K.sh);
    count_bytes(2.0 * a->limbs, a->batch);
}
CtPtr Engine::mul_int(const Ciphertext &a, i64 K) {
    const size_t ln = a.limbs * n();
    auto r = new_ct(a.level, a.slots, a.scale, a.limbs, a.batch);
    dev::ew_mul_scalar(r->data, a.data, K, (int)a.limbs, 2 * a.batch, seg3(ln, ln, 0), MODS, LOGN, ST);
    count_bytes(4.0 * a.limbs, a.batch);
    return r;
}
CtPtr Engine::mul_const_to(const Ciphertext &a, double c, int target) {
    auto &I = *impl;
    if (target <= a.level) throw std::invalid_argument("mul_const_to: target must exceed level");
    if (target > I.P.L) throw std::runtime_error("mul_const_to: no levels left");
    ctr.constmult += a.batch;
    ctr.rescale += a.batch;
    const size_t nn = n(), ell = I.P.limbs_at(target - 1);
    count_bytes(4.0 * ell, a.batch);
    const host::SConst K = host::const_to_target(c, I.P.delta[target], I.P.primes[I.P.L - target + 1], a.scale);
    const int segs = 2 * a.batch;
    auto r = new_ct(target, a.slots, I.P.delta[target], ell - 1, a.batch);
    if (K.k == 0) {  // rescale(0 * a) = 0
        HIP_OK(hipMemsetAsync(r->data, 0, (size_t)segs * (ell - 1) * nn * 8, ST));
        return r;
    }
    // Rescale(K * a) of the first ell limbs, K folded into the fused NTT
    I.rescale(a.data, ell, a.limbs * nn, segs, r->data, K);
    return r;
}
CtPtr Engine::mul_const(const Ciphertext &a, double c) { return mul_const_to(a, c, a.level + 1); }
CtPtr Engine::level_adjust(const Ciphertext &a, int target) {
    if (target == a.level) return clone(a);
    return mul_const_to(a, 1.0, target);
}
CtPtr Engine::rescale(const Ciphertext &a) {
    auto &I = *impl;
    if (a.level >= I.P.L) throw std::runtime_error("rescale: no levels left");
    ctr.rescale += a.batch;
    count_bytes(4.0 * a.limbs, a.batch);
    auto r = new_ct(a.level + 1, a.slots, a.scale / (double)I.P.primes[a.limbs - 1], a.limbs - 1, a.batch);
    I.rescale(a.data, a.limbs, a.limbs * n(), 2 * a.batch, r->data);
    return r;
}
CtPtr Engine::mul_plain(const Ciphertext &a, const Plaintext &p) {
    auto &I = *impl;
    if (p.level != a.level) throw std::invalid_argument("mul_plain: level mismatch");
    if (a.level >= I.P.L) throw std::runtime_error("mul_plain: no levels left");
    ctr.ptmult += a.batch;
    ctr.rescale += a.batch;
    const size_t nn = n(), ell = a.limbs;
    count_bytes(5.0 * ell, a.batch);
    const int segs = 2 * a.batch;
    auto tm = I.alloc((size_t)segs * ell * nn * 8);
    u64 *t = static_cast<u64 *>(tm->p);
    dev::ew_mul_plain(t, a.data, p.data, (int)ell, segs, seg3(ell * nn, ell * nn, 0), MODS, LOGN, ST);
    auto r = new_ct(a.level + 1, a.slots, I.P.delta[a.level + 1], ell - 1, a.batch);
    I.rescale(t, ell, ell * nn, segs, r->data);
    return r;
}

// sum_i a_i * p_i with one rescale (the oracle's spec; OpenFHE's FLEXIBLEAUTO
// also rescales a masked sum once).  All a_i share level and batch.
CtPtr Engine::mul_plain_sum(const std::vector<const Ciphertext *> &a, const std::vector<const Plaintext *> &p) {
    auto &I = *impl;
    if (a.empty() || a.size() != p.size()) throw std::invalid_argument("mul_plain_sum: bad operand lists");
    const int level = a[0]->level, B = a[0]->batch;
    for (size_t i = 0; i < a.size(); ++i) {
        if (a[i]->level != level || p[i]->level != level)
            throw std::invalid_argument("mul_plain_sum: level mismatch");
        if (a[i]->batch != B) throw std::invalid_argument("mul_plain_sum: batch size mismatch");
    }
    if (level >= I.P.L) throw std::runtime_error("mul_plain_sum: no levels left");
    ctr.ptmult += a.size() * B;
    ctr.rescale += B;
    const size_t nn = n(), ell = a[0]->limbs;
    count_bytes(2.0 * ell * a.size() + 2.0 * ell, B);  // the ct reads and the output
    count_bytes((double)ell * a.size(), 1);            // the shared plaintexts
    std::vector<const u64 *> cp, pp;
    for (size_t i = 0; i < a.size(); ++i) {
        cp.push_back(a[i]->data);
        pp.push_back(p[i]->data);
    }
    auto tm = I.alloc((size_t)2 * B * ell * nn * 8);
    u64 *t = static_cast<u64 *>(tm->p);
    dev::ew_mul_plain_sum(t, cp.data(), pp.data(), (int)a.size(), (int)ell, B, 2 * ell * nn, ell * nn, MODS, LOGN, ST);
    auto r = new_ct(level + 1, a[0]->slots, I.P.delta[level + 1], ell - 1, B);
    I.rescale(t, ell, ell * nn, 2 * B, r->data);
    return r;
}

// FHE_RANK_STACK_MASKS (A/B, default 1): the masked sums of a chunk's batches in
// one pass over the shared ciphertexts; 0: one mul_plain_sum per batch, stacked
static bool stack_masks_enabled() {
    static const bool on = env_switch("FHE_RANK_STACK_MASKS", 1);
    return on;
}

// member b = sum_i a_i * p[b][i] with one rescale: nb mul_plain_sum calls over
// the same single ciphertexts, word for word, with their counters and op bytes
CtPtr Engine::mul_plain_sum_batches(const std::vector<const Ciphertext *> &a,
                                    const std::vector<std::vector<const Plaintext *>> &p) {
    auto &I = *impl;
    if (a.empty() || p.empty()) throw std::invalid_argument("mul_plain_sum_batches: bad operand lists");
    const int level = a[0]->level, nb = (int)p.size();
    const size_t m = a.size();
    for (size_t i = 0; i < m; ++i) {
        if (a[i]->level != level) throw std::invalid_argument("mul_plain_sum_batches: level mismatch");
        if (a[i]->batch != 1) throw std::invalid_argument("mul_plain_sum_batches: single ciphertexts only");
    }
    for (auto &row : p) {
        if (row.size() != m) throw std::invalid_argument("mul_plain_sum_batches: bad operand lists");
        for (auto *pt : row)
            if (pt->level != level) throw std::invalid_argument("mul_plain_sum_batches: level mismatch");
    }
    if (level >= I.P.L) throw std::runtime_error("mul_plain_sum_batches: no levels left");
    if (!stack_masks_enabled()) {
        std::vector<CtPtr> T;
        std::vector<const Ciphertext *> tp;
        for (auto &row : p) {
            T.push_back(mul_plain_sum(a, row));
            tp.push_back(T.back().get());
        }
        return stack(tp);
    }
    const size_t nn = n(), ell = a[0]->limbs;
    for (int b = 0; b < nb; ++b) {  // what nb mul_plain_sum calls book
        ctr.ptmult += m;
        ctr.rescale += 1;
        count_bytes(2.0 * ell * m + 2.0 * ell, 1);
        count_bytes((double)ell * m, 1);
    }
    std::vector<const u64 *> cp, pp;
    for (size_t i = 0; i < m; ++i) cp.push_back(a[i]->data);
    for (auto &row : p)
        for (auto *pt : row) pp.push_back(pt->data);
    auto tm = I.alloc((size_t)2 * nb * ell * nn * 8);
    u64 *t = static_cast<u64 *>(tm->p);
    dev::ew_mul_plain_sum_batches(t, cp.data(), I.ptr_table(pp), (int)m, nb, (int)ell, ell * nn, MODS, LOGN, ST);
    auto r = new_ct(level + 1, a[0]->slots, I.P.delta[level + 1], ell - 1, nb);
    I.rescale(t, ell, ell * nn, 2 * nb, r->data);
    return r;
}

// FHE_SELECT_FUSED (A/B, default 1): mul_plain_sum_groups' sums of every group in
// one pass over the shared plaintexts; 0: one mul_plain_sum per group, stacked
static bool select_fused_enabled() {
    static const bool on = env_switch("FHE_SELECT_FUSED", 1);
    return on;
}

// member g = sum_z a[g Z + z] * p[z] with one rescale: `groups` mul_plain_sum
// calls over the same plaintexts, word for word, with their counters and op bytes
CtPtr Engine::mul_plain_sum_groups(const Ciphertext &a, const std::vector<const Plaintext *> &p, int groups) {
    auto &I = *impl;
    if (p.empty() || groups < 1 || groups > 32767 || (size_t)a.batch != p.size() * (size_t)groups)
        throw std::invalid_argument("mul_plain_sum_groups: the stack is not `groups` groups of one member per plaintext");
    const int level = a.level, Z = (int)p.size();
    for (auto *pt : p)
        if (!pt || pt->level != level) throw std::invalid_argument("mul_plain_sum_groups: level mismatch");
    if (level >= I.P.L) throw std::runtime_error("mul_plain_sum_groups: no levels left");
    if (!select_fused_enabled()) {
        std::vector<CtPtr> T, views;
        std::vector<const Ciphertext *> tp;
        for (int g = 0; g < groups; ++g) {
            std::vector<const Ciphertext *> ms;
            for (int z = 0; z < Z; ++z) {
                views.push_back(member(a, g * Z + z));
                ms.push_back(views.back().get());
            }
            T.push_back(mul_plain_sum(ms, p));
            tp.push_back(T.back().get());
        }
        return groups == 1 ? T[0] : stack(tp);
    }
    const size_t nn = n(), ell = a.limbs;
    for (int g = 0; g < groups; ++g) {  // what `groups` mul_plain_sum calls book
        ctr.ptmult += Z;
        ctr.rescale += 1;
        count_bytes(2.0 * ell * Z + 2.0 * ell, 1);
        count_bytes((double)ell * Z, 1);
    }
    std::vector<const u64 *> pp;
    for (auto *pt : p) pp.push_back(pt->data);
    auto tm = I.alloc((size_t)2 * groups * ell * nn * 8);
    u64 *t = static_cast<u64 *>(tm->p);
    dev::ew_mul_plain_sum_groups(t, a.data, pp.data(), Z, groups, (int)ell, MODS, LOGN, ST);
    auto r = new_ct(level + 1, a.slots, I.P.delta[level + 1], ell - 1, groups);
    I.rescale(t, ell, ell * nn, 2 * groups, r->data);
    return r;
}

// FHE_TENSOR_LIN (A/B, default 1): mul_add's summands folded into the tensor pass
static bool tensor_lin_enabled() {
    static const bool on = env_switch("FHE_TENSOR_LIN", 1);
    return on;
}

// FHE_MUL_FOLD_CONST (A/B, default 1): mul_add's a_const added on load in the
// tensor pass and its out_const there as a term of d0; 0: the separate
// add_const / add_const_inplace launches.  Same words either way.
static bool mul_fold_const() {
    static const bool on = env_switch("FHE_MUL_FOLD_CONST", 1);
    return on;
}

// ct x ct with relinearisation and rescale.  b may be a single ciphertext
// multiplied into every member of a (broadcast).
CtPtr Engine::mul(const Ciphertext &a0, const Ciphertext &b0) { return mul_add(a0, b0, {}, {}); }

// a*b + sum_i c_i x_i with one rescale: the sum is formed at the product's
// pre-rescale scale (the constants of linear_sum_to(xs, c, level+1)) and added
// to the tensor's (d0, d1) before relinearisation (oracle: Context::mul_add).
CtPtr Engine::mul_add(const Ciphertext &a0, const Ciphertext &b0, const std::vector<const Ciphertext *> &xs,
                      const std::vector<double> &cs, const Ciphertext *raw, const Ciphertext *a_add, double a_const,
                      double out_const) {
    auto &I = *impl;
    if (a0.batch != b0.batch && b0.batch != 1) throw std::invalid_argument("mul: batch size mismatch");
    // a + a_add fused into the tensor pass only where add() would not level-adjust
    // and the sum would not be level-adjusted against b; otherwise formed first
    if (a_add && (a_add->level != a0.level || a_add->batch != a0.batch || a0.level < b0.level)) {
        CtPtr s = add(a0, *a_add);
        if (a_const != 0.0) s = add_const(*s, a_const);
        return mul_add(*s, b0, xs, cs, raw, nullptr, 0.0, out_const);
    }
    // + a_const on load likewise only where add_const would see this operand
    // (mul_fold_left); + out_const as a term of d0 unless switched off
    if (a_const != 0.0 && !mul_fold_left(mul_fold_const(), a0.level, b0.level))
        return mul_add(*add_const(a0, a_const), b0, xs, cs, raw, a_add, 0.0, out_const);
    if (out_const != 0.0 && !mul_fold_const()) {
        CtPtr r = mul_add(a0, b0, xs, cs, raw, a_add, a_const, 0.0);
        add_const_inplace(r, out_const);
        return r;
    }
    auto a = std::make_shared<Ciphertext>(a0), b = std::make_shared<Ciphertext>(b0);
    match_levels(a, b);
    if (a->level >= I.P.L) throw std::runtime_error("mul: no levels left");
    if (!I.ks->relin) throw std::runtime_error("mul: no relinearisation key");
    const int B = a->batch;
    ctr.hmult += B;
    ctr.keyswitch += B;
    ctr.rescale += B;
    const size_t nn = n(), ell = a->limbs;
    count_bytes(6.0 * ell + ks_units(ell) + 2.0 * ell * xs.size(), B);
    auto d01m = I.alloc((size_t)B * 2 * ell * nn * 8), d2m = I.alloc((size_t)B * ell * nn * 8);
    u64 *d01 = static_cast<u64 *>(d01m->p), *d2 = static_cast<u64 *>(d2m->p);
    if (a_add) count_bytes(6.0 * ell, B);  // the add it replaces
    // the constant steps they replace: add_const's copy, add_const_inplace's c0 pass
    const host::SConst Ka = a_const != 0.0 ? host::const_at_scale(a_const, a->scale) : host::SConst{};
    const host::SConst Ko = out_const != 0.0 ? host::const_at_scale(out_const, I.P.delta[a->level + 1]) : host::SConst{};
    if (a_const != 0.0) count_bytes(4.0 * ell, B);
    if (out_const != 0.0) count_bytes(2.0 * (ell - 1), B);
    // the summands folded into the tensor pass (k_tensor_lin) when they share a
    // limb count and are at most four: no second pass over d01
    bool fused_lin = false;
    if (!xs.empty() && xs.size() <= 4 && tensor_lin_enabled()) {
        const int target = a->level + 1;
        const u64 qd = I.P.primes[I.P.L - target + 1];
        std::vector<const u64 *> x;
        std::vector<int64_t> k;
        std::vector<uint8_t> sh;
        bool one = true;
        for (size_t i = 0; i < xs.size(); ++i) {
            if (xs[i]->level > a->level) throw std::invalid_argument("mul_add: summand level too high");
            if (xs[i]->batch != B) throw std::invalid_argument("mul_add: batch size mismatch");
            one = one && xs[i]->limbs == xs[0]->limbs;
            const host::SConst K = host::const_to_target(cs[i], I.P.delta[target], qd, xs[i]->scale);
            x.push_back(xs[i]->data);
            k.push_back(K.k);
            sh.push_back((uint8_t)K.sh);
        }
        if (one)
            fused_lin = dev::ew_tensor_lin(d01, d2, a->data, b->data, (int)ell, B, 2 * ell * nn,
                                           b->batch == 1 ? 0 : 2 * ell * nn, x.data(), k.data(), sh.data(),
                                           (int)x.size(), xs[0]->limbs * nn, MODS, LOGN, ST,
                                           a_add ? a_add->data : nullptr, 2 * ell * nn, Ka.k, Ka.sh, Ko.k, Ko.sh);
        if (fused_lin) ctr.constmult += xs.size() * B;
    }
    // a raw summand alone rides the tensor pass as a summand with constant one
    // (mul_mod(x, 1) = x and the sum is reduced once: add_mod's words) instead of
    // a k_add pass over d01 behind it
    bool fused_raw = false;
    if (raw && (raw->level != a->level || raw->limbs != ell || raw->batch != B))
        throw std::invalid_argument("mul_add: raw summand shape mismatch");
    if (raw && xs.empty() && tensor_lin_enabled() && mul_fold_const()) {
        const u64 *x = raw->data;
        const int64_t k = 1;
        const uint8_t sh = 0;
        fused_raw = dev::ew_tensor_lin(d01, d2, a->data, b->data, (int)ell, B, 2 * ell * nn,
                                       b->batch == 1 ? 0 : 2 * ell * nn, &x, &k, &sh, 1, ell * nn, MODS, LOGN, ST,
                                       a_add ? a_add->data : nullptr, 2 * ell * nn, Ka.k, Ka.sh, Ko.k, Ko.sh);
    }
    if (!fused_lin && !fused_raw)
        dev::ew_tensor(d01, d2, a->data, b->data, (int)ell, B, 2 * ell * nn, b->batch == 1 ? 0 : 2 * ell * nn, MODS,
                       LOGN, ST, a_add ? a_add->data : nullptr, 2 * ell * nn, Ka.k, Ka.sh, Ko.k, Ko.sh);
    if (!xs.empty() && !fused_lin) {
        const int target = a->level + 1;
        const u64 qd = I.P.primes[I.P.L - target + 1];
        struct Group {
            std::vector<const u64 *> x;
            std::vector<int64_t> k;
            std::vector<uint8_t> sh;
        };
        std::map<size_t, Group> by_limbs;
        for (size_t i = 0; i < xs.size(); ++i) {
            if (xs[i]->level > a->level) throw std::invalid_argument("mul_add: summand level too high");
            if (xs[i]->batch != B) throw std::invalid_argument("mul_add: batch size mismatch");
            auto &g = by_limbs[xs[i]->limbs];
            const host::SConst K = host::const_to_target(cs[i], I.P.delta[target], qd, xs[i]->scale);
            g.x.push_back(xs[i]->data);
            g.k.push_back(K.k);
            g.sh.push_back((uint8_t)K.sh);
        }
        for (auto &kv : by_limbs)
            dev::ew_linear_sum(d01, kv.second.x.data(), kv.second.k.data(), (int)kv.second.x.size(), (int)ell, 2 * B,
                               ell * nn, kv.first * nn, MODS, LOGN, ST, true, kv.second.sh.data());
        ctr.constmult += xs.size() * B;
    }
    if (raw && !fused_raw) {
        const size_t ln = ell * nn;
        dev::ew_add(d01, d01, raw->data, (int)ell, 2 * B, dev::Seg{ln, ln, ln}, MODS, LOGN, ST);
    }
    const bool fuse = I.ks_fuse(B);
    auto extm = I.modup(d2, ell, B, ell * nn, fuse);
    auto r = new_ct(a->level + 1, a->slots, I.P.delta[a->level + 1], ell - 1, B);
    I.mul_tail(static_cast<u64 *>(extm->p), d01, d2, ell, B, r->data, fuse);
    return r;
}
CtPtr Engine::mul_add_raw(const Ciphertext &a, const Ciphertext &b, const Ciphertext &raw, const Ciphertext *a_add,
                          double a_const, double out_const) {
    return mul_add(a, b, {}, {}, &raw, a_add, a_const, out_const);
}
CtPtr Engine::square(const Ciphertext &a) { return mul(a, a); }

// FHE_SORT_COLS_FUSED (A/B, default 1): mul_columns' tensor of every column in one pass
static bool cols_fused_enabled() {
    static const bool on = env_switch("FHE_SORT_COLS_FUSED", 1);
    return on;
}

CtPtr Engine::mul_columns(const Ciphertext &a, const std::vector<const Ciphertext *> &cols) {
    if (cols.empty()) throw std::invalid_argument("mul_columns: no columns");
    for (size_t p = 0; p < cols.size(); ++p) {
        if (!cols[p]) throw std::invalid_argument("mul_columns: column " + std::to_string(p) + " is null");
        if (cols[p]->batch != 1)
            throw std::invalid_argument("mul_columns: column " + std::to_string(p) + " is a stack");
        if (cols[p]->level > a.level)
            throw std::invalid_argument("mul_columns: column " + std::to_string(p) + " is at a higher level than a");
    }
    if (!cols_fused_enabled()) {
        std::vector<CtPtr> prod;
        std::vector<const Ciphertext *> v;
        for (auto *c : cols) {
            prod.push_back(mul(a, *c));
            v.push_back(prod.back().get());
        }
        return prod.size() == 1 ? prod[0] : stack(v);
    }
    const int B = a.batch, Pn = (int)cols.size(), PB = Pn * B;
    const size_t nn = n(), ell = a.limbs;
    return product_tail(a, PB, [&](u64 *d01, u64 *d2) {
        std::vector<CtPtr> adj;  // the columns mul would level-adjust, kept until the tensor pass is enqueued
        std::vector<const u64 *> cp;
        for (auto *c : cols) {
            if (c->level < a.level) {
                adj.push_back(level_adjust(*c, a.level));
                c = adj.back().get();
            }
            if (c->limbs != a.limbs) throw std::invalid_argument("mul_columns: limb count mismatch");
            cp.push_back(c->data);
        }
        count_bytes(6.0 * ell + ks_units(ell), PB);
        dev::ew_tensor_cols(d01, d2, a.data, cp.data(), Pn, (int)ell, B, 2 * ell * nn, MODS, LOGN, ST);
    });
}

// FHE_GROUP_FUSED (A/B, default 1): the one-pass kernels of mul_pairs and sub_pm_const_stacked
static bool group_fused_enabled() {
    static const bool on = env_switch("FHE_GROUP_FUSED", 1);
    return on;
}

CtPtr Engine::mul_pairs(const Ciphertext &a, const Ciphertext &a_add, const Ciphertext &b, int Pn) {
    if (Pn < 1) throw std::invalid_argument("mul_pairs: no columns");
    if (a.batch < 1 || a_add.batch != a.batch)
        throw std::invalid_argument("mul_pairs: a and a_add differ in member count");
    if (a_add.level != a.level || a_add.limbs != a.limbs)
        throw std::invalid_argument("mul_pairs: a and a_add differ in level");
    if ((long long)b.batch != (long long)Pn * a.batch)
        throw std::invalid_argument("mul_pairs: b holds " + std::to_string(b.batch) + " members, need " +
                                    std::to_string(Pn) + " columns of " + std::to_string(a.batch));
    if (b.level != a.level || b.limbs != a.limbs) throw std::invalid_argument("mul_pairs: b is not at a's level");
    const int B = a.batch, PB = Pn * B;
    const size_t nn = n(), ell = a.limbs;
    if (!group_fused_enabled()) {  // the plain form (A/B): one mul_add with a_add per column, stacked
        std::vector<CtPtr> prod;
        std::vector<const Ciphertext *> v;
        for (int p = 0; p < Pn; ++p) {
            Ciphertext col = b;
            col.data = b.data + (size_t)p * B * 2 * ell * nn;
            col.batch = B;
            prod.push_back(mul_add(a, col, {}, {}, nullptr, &a_add));
            v.push_back(prod.back().get());
        }
        return prod.size() == 1 ? prod[0] : stack(v);
    }
    return product_tail(a, PB, [&](u64 *d01, u64 *d2) {
        count_bytes(5.0 * ell + ks_units(ell), PB);
        const int per = dev::TENSOR_TILE;
        count_bytes(4.0 * ell * ((Pn + per - 1) / per), B);
        dev::ew_tensor_pairs(d01, d2, a.data, a_add.data, b.data, Pn, (int)ell, B, 2 * ell * nn, MODS, LOGN, ST);
    });
}

std::vector<CtPtr> Engine::rotate_hoisted(const Ciphertext &a, const std::vector<long> &ks) {
    auto &I = *impl;
    std::vector<u64> gs;
    for (long k : ks) {
        const u64 g = host::galois_for_rotation(I.P.logN, k);
        if (g != 1 && !I.ks->rotkeys.count(g)) throw NoKeyError("rotate: no rotation key for index " + std::to_string(k));
        gs.push_back(g);
    }
    return apply_galois_hoisted(a, gs);
}
CtPtr Engine::conjugate(const Ciphertext &a) { return apply_galois_hoisted(a, {2 * (u64)n() - 1})[0]; }

std::vector<CtPtr> Engine::apply_galois_hoisted(const Ciphertext &a, const std::vector<u64> &gs) {
    auto &I = *impl;
    const size_t nn = n(), ell = a.limbs, ln = ell * nn;
    const int B = a.batch;
    std::vector<CtPtr> outs;
    std::shared_ptr<DevMem> extm;
    size_t keyed = 0;
    for (u64 g : gs) keyed += g != 1;
    if (B == 1 && keyed >= 2) {
        // one ModUp, then every key switch, c0 permutation and ModDown of the
        // set in the same launches (outputs are members of one batch)
        std::vector<size_t> slot(gs.size(), (size_t)-1);
        std::vector<u64> kg;
        for (size_t i = 0; i < gs.size(); ++i) {
            if (gs[i] == 1) continue;
            if (!I.ks->rotkeys.count(gs[i]))
                throw NoKeyError("rotate: no key for galois element " + std::to_string(gs[i]));
            slot[i] = kg.size();
            kg.push_back(gs[i]);
        }
        extm = I.modup(a.data + ln, ell, 1, 2 * ln);
        auto r = new_ct(a.level, a.slots, a.scale, ell, (int)kg.size());
        auto c0m = I.alloc(kg.size() * ln * 8);
        u64 *c0p = static_cast<u64 *>(c0m->p);
        for (size_t c0 = 0; c0 < kg.size(); c0 += dev::KS_MAXKEYS) {
            const int cnt = (int)std::min<size_t>(dev::KS_MAXKEYS, kg.size() - c0);
            dev::KsKeys KK{};
            for (int i = 0; i < cnt; ++i) {
                KK.key[i] = static_cast<const u64 *>(I.ks->rotkeys.at(kg[c0 + i])->p);
                KK.perm[i] = I.perm(kg[c0 + i]);
            }
            dev::ew_permute_multi(c0p + c0 * ln, a.data, KK, (int)ell, cnt, seg3(ln, 0, 0), LOGN, ST);
            I.ks_apply_multi(static_cast<u64 *>(extm->p), 0, a.data + ln, 0, ell, cnt, KK, r->data + c0 * 2 * ln,
                             c0p + c0 * ln, ln);
        }
        ctr.keyswitch += kg.size();
        ctr.rotations += kg.size();
        count_bytes((4.0 * ell + ks_units(ell)) * (double)kg.size(), 1);
        for (size_t i = 0; i < gs.size(); ++i) outs.push_back(slot[i] == (size_t)-1 ? clone(a) : member(*r, (int)slot[i]));
        return outs;
    }
    for (u64 g : gs) {
        if (g == 1) {
            outs.push_back(clone(a));
            continue;
        }
        auto it = I.ks->rotkeys.find(g);
        if (it == I.ks->rotkeys.end()) throw NoKeyError("rotate: no key for galois element " + std::to_string(g));
        if (!extm) extm = I.modup(a.data + ln, ell, B, 2 * ln);  // c1 of every member
        ctr.keyswitch += B;
        ctr.rotations += B;
        count_bytes(4.0 * ell + ks_units(ell), B);
        const uint32_t *pm = I.perm(g);
        auto c0m = I.alloc((size_t)B * ln * 8);
        u64 *c0p = static_cast<u64 *>(c0m->p);
        dev::ew_permute(c0p, a.data, pm, (int)ell, B, seg3(ln, 2 * ln, 0), LOGN, ST);
        auto r = new_ct(a.level, a.slots, a.scale, ell, B);
        I.ks_apply(static_cast<u64 *>(extm->p), a.data + ln, 2 * ln, ell, B, static_cast<u64 *>(it->second->p), pm,
                   r->data, c0p, ln);
        outs.push_back(r);
    }
    return outs;
}
CtPtr Engine::rotate(const Ciphertext &a, long k) { return rotate_hoisted(a, {k})[0]; }

// member m of `a` rotated by ks[m] (every ks[m] keyed, i.e. not 0 mod n/2): one
// ModUp of all members, then the key switches in the same launches
CtPtr Engine::rotate_members(const Ciphertext &a, const std::vector<long> &ks) {
    auto &I = *impl;
    if ((int)ks.size() != a.batch) throw std::invalid_argument("rotate_members: one rotation per member");
    const size_t nn = n(), ell = a.limbs, ln = ell * nn;
    const int B = a.batch;
    std::vector<u64> gs;
    for (long k : ks) {
        const u64 g = host::galois_for_rotation(I.P.logN, k);
        if (g == 1) throw std::invalid_argument("rotate_members: identity rotation");
        if (!I.ks->rotkeys.count(g)) throw NoKeyError("rotate: no rotation key for index " + std::to_string(k));
        gs.push_back(g);
    }
    auto extm = I.modup(a.data + ln, ell, B, 2 * ln);
    const size_t es = (size_t)I.P.digits_at(ell) * (ell + I.P.K) * nn;
    auto r = new_ct(a.level, a.slots, a.scale, ell, B);
    auto c0m = I.alloc((size_t)B * ln * 8);
    u64 *c0p = static_cast<u64 *>(c0m->p);
    for (int c0 = 0; c0 < B; c0 += dev::KS_MAXKEYS) {
        const int cnt = std::min(dev::KS_MAXKEYS, B - c0);
        dev::KsKeys KK{};
        for (int i = 0; i < cnt; ++i) {
            KK.key[i] = static_cast<const u64 *>(I.ks->rotkeys.at(gs[c0 + i])->p);
            KK.perm[i] = I.perm(gs[c0 + i]);
        }
        dev::ew_permute_multi(c0p + c0 * ln, a.data + c0 * 2 * ln, KK, (int)ell, cnt, seg3(ln, 2 * ln, 0), LOGN, ST);
        I.ks_apply_multi(static_cast<u64 *>(extm->p) + c0 * es, es, a.data + c0 * 2 * ln + ln, 2 * ln, ell, cnt, KK,
                         r->data + c0 * 2 * ln, c0p + c0 * ln, ln);
    }
    ctr.keyswitch += B;
    ctr.rotations += B;
    count_bytes(4.0 * ell + ks_units(ell), B);
    return r;
}

CtPtr Engine::rotate_sum_hoisted(const Ciphertext &x, const std::vector<long> &ks) {
    auto &I = *impl;
    if (ks.empty()) return clone(x);
    const size_t nn = n(), ell = x.limbs, ln = ell * nn, W = ell + (size_t)I.P.K;
    const int digits = I.P.digits_at(ell), B = x.batch;
    std::vector<u64> gs;
    for (long k : ks) {
        const u64 g = host::galois_for_rotation(I.P.logN, k);
        if (g == 1) throw std::invalid_argument("rotate_sum_hoisted: identity rotation");
        if (!I.ks->rotkeys.count(g)) throw NoKeyError("rotate: no rotation key for index " + std::to_string(k));
        gs.push_back(g);
    }
    // a stack: member m's ModUp at m * es, its accumulator pair at m * 2 W n, its c0 sum at m * ln
    auto extm = I.modup(x.data + ln, ell, B, 2 * ln);
    auto accm = I.alloc((size_t)B * 2 * W * nn * 8), c0m = I.alloc((size_t)B * ln * 8);
    u64 *acc = static_cast<u64 *>(accm->p), *c0 = static_cast<u64 *>(c0m->p);
    dev::KsStrides str;  // every rotation reads the one hoisted ModUp and x's c1
    dev::MbStrides mb;
    mb.out = 2 * W * nn;
    mb.ext = (size_t)digits * W * nn;
    mb.c = 2 * ln;
    for (size_t b0 = 0; b0 < gs.size(); b0 += dev::KS_MAXKEYS) {
        const int cnt = (int)std::min<size_t>(dev::KS_MAXKEYS, gs.size() - b0);
        dev::KsKeys KK{};
        for (int i = 0; i < cnt; ++i) {
            KK.key[i] = static_cast<const u64 *>(I.ks->rotkeys.at(gs[b0 + i])->p);
            KK.perm[i] = I.perm(gs[b0 + i]);
        }
        if (B == 1) {
            dev::ew_permute_sum(c0, x.data, KK, (int)ell, cnt, b0 > 0, 0, MODS, LOGN, ST);
            dev::ks_inner_multikey_sum(acc, static_cast<u64 *>(extm->p), x.data + ln, KK, cnt, b0 > 0, (int)ell, I.P.K,
                                       (int)I.P.nall(), I.P.alpha, digits, I.ext(ell), MODS, LOGN, ST, str);
        } else {
            dev::ew_permute_sum_members(c0, x.data, KK, (int)ell, cnt, b0 > 0, 0, B, ln, 2 * ln, MODS, LOGN, ST);
            dev::ks_inner_multikey_sum_members(acc, static_cast<u64 *>(extm->p), x.data + ln, KK, cnt, b0 > 0, (int)ell,
                                               I.P.K, (int)I.P.nall(), I.P.alpha, digits, B, mb, I.ext(ell), MODS, LOGN,
                                               ST, str);
        }
    }
    auto t = new_ct(x.level, x.slots, x.scale, ell, B);
    I.ks_moddown(acc, ell, 2 * B, t->data, c0, ln);
    dev::ew_add(t->data, t->data, x.data, (int)ell, 2 * B, seg3(ln, ln, ln), MODS, LOGN, ST);
    ctr.keyswitch += gs.size() * B;
    ctr.rotations += gs.size() * B;
    count_bytes((4.0 * ell + ks_units(ell)) * (double)gs.size() + 6.0 * ell, B);
    return t;
}

CtPtr Engine::linear_transform_ext(const Ciphertext &x, const std::vector<long> &baby,
                                   const std::vector<LtGiant> &giants) {
    auto &I = *impl;
    if (x.level >= I.P.L) throw std::runtime_error("linear_transform_ext: no levels left");
    const size_t nn = n(), ell = x.limbs, ln = ell * nn, W = ell + (size_t)I.P.K;
    const int digits = I.P.digits_at(ell), B = x.batch;
    std::vector<const u64 *> bkey(baby.size(), nullptr);
    std::vector<const uint32_t *> bperm(baby.size(), nullptr);
    size_t keyed = 0;
    for (size_t b = 0; b < baby.size(); ++b) {
        const u64 g = host::galois_for_rotation(I.P.logN, baby[b]);
        if (g == 1) continue;
        auto it = I.ks->rotkeys.find(g);
        if (it == I.ks->rotkeys.end()) throw NoKeyError("rotate: no rotation key for index " + std::to_string(baby[b]));
        bkey[b] = static_cast<const u64 *>(it->second->p);
        bperm[b] = I.perm(g);
        ++keyed;
    }
    // a stack: every per-ciphertext buffer below holds B of them, member-major
    const size_t es = (size_t)digits * W * nn, as = 2 * W * nn;
    dev::MbStrides mb;
    mb.out = as;
    mb.ext = es;
    mb.c = 2 * ln;
    auto extm = I.modup(x.data + ln, ell, B, 2 * ln);
    const u64 *ext = static_cast<const u64 *>(extm->p);
    size_t npt = 0;
    auto inner_of = [&](const LtGiant &G, u64 *out) {
        if (G.baby.empty() || G.baby.size() != G.pts.size())
            throw std::invalid_argument("linear_transform_ext: one plaintext per baby");
        for (size_t b0 = 0; b0 < G.baby.size(); b0 += dev::LT_MAXB) {
            dev::LtArgs A{};
            A.nb = (int)std::min<size_t>(dev::LT_MAXB, G.baby.size() - b0);
            for (int i = 0; i < A.nb; ++i) {
                const int bi = G.baby[b0 + i];
                const Plaintext *p = G.pts[b0 + i];
                if (bi < 0 || (size_t)bi >= baby.size()) throw std::invalid_argument("linear_transform_ext: bad baby index");
                if (p->limbs != W || p->level != x.level)
                    throw std::invalid_argument("linear_transform_ext: plaintexts must be extended, at the input's level");
                A.key[i] = bkey[(size_t)bi];
                A.perm[i] = bperm[(size_t)bi];
                A.pt[i] = p->data;
            }
            if (B == 1)
                dev::lt_inner(out, ext, x.data, A, b0 > 0, (int)ell, I.P.K, (int)I.P.nall(), I.P.alpha, digits,
                              I.ext(ell), I.pmod, I.pmod_s, MODS, LOGN, ST);
            else
                dev::lt_inner_members(out, ext, x.data, A, b0 > 0, (int)ell, I.P.K, (int)I.P.nall(), I.P.alpha, digits, B,
                                      mb, I.ext(ell), I.pmod, I.pmod_s, MODS, LOGN, ST);
        }
        npt += G.baby.size();
    };
    auto accm = I.alloc((size_t)B * as * 8);
    u64 *acc = static_cast<u64 *>(accm->p);
    bool have_acc = false;
    std::vector<const LtGiant *> shifted;
    for (const LtGiant &G : giants) {
        if (G.shift != 0) {
            shifted.push_back(&G);
            continue;
        }
        if (have_acc) throw std::invalid_argument("linear_transform_ext: two unrotated giants");
        inner_of(G, acc);
        have_acc = true;
    }
    std::shared_ptr<DevMem> c0m;
    const int S = (int)shifted.size();
    if (S > 0) {
        // each rotated giant's inner sum brought down to Q, then all of them
        // rotated with their key products summed into acc.  q holds giant i of
        // member m at (i B + m) * 2 ln, so one ModUp serves the S B inputs
        auto qm = I.alloc((size_t)S * B * 2 * ln * 8), tm = I.alloc((size_t)B * as * 8);
        u64 *q = static_cast<u64 *>(qm->p), *tmp = static_cast<u64 *>(tm->p);
        std::vector<u64> gs;
        for (int i = 0; i < S; ++i) {
            inner_of(*shifted[(size_t)i], tmp);
            I.ks_moddown(tmp, ell, 2 * B, q + (size_t)i * B * 2 * ln, nullptr, 0);
            const u64 g = host::galois_for_rotation(I.P.logN, shifted[(size_t)i]->shift);
            if (g == 1 || !I.ks->rotkeys.count(g))
                throw NoKeyError("rotate: no rotation key for index " + std::to_string(shifted[(size_t)i]->shift));
            gs.push_back(g);
        }
        auto ext2 = I.modup(q + ln, ell, S * B, 2 * ln);
        c0m = I.alloc((size_t)B * ln * 8);
        u64 *c0 = static_cast<u64 *>(c0m->p);
        dev::KsStrides str;
        str.ext = (size_t)B * es;
        str.d = (size_t)B * 2 * ln;
        for (int b0 = 0; b0 < S; b0 += dev::KS_MAXKEYS) {
            const int cnt = std::min(dev::KS_MAXKEYS, S - b0);
            dev::KsKeys KK{};
            for (int i = 0; i < cnt; ++i) {
                KK.key[i] = static_cast<const u64 *>(I.ks->rotkeys.at(gs[(size_t)(b0 + i)])->p);
                KK.perm[i] = I.perm(gs[(size_t)(b0 + i)]);
            }
            const u64 *qb = q + (size_t)b0 * str.d, *eb = static_cast<u64 *>(ext2->p) + (size_t)b0 * str.ext;
            if (B == 1) {
                dev::ew_permute_sum(c0, qb, KK, (int)ell, cnt, b0 > 0, 2 * ln, MODS, LOGN, ST);
                dev::ks_inner_multikey_sum(acc, eb, qb + ln, KK, cnt, have_acc || b0 > 0, (int)ell, I.P.K,
                                           (int)I.P.nall(), I.P.alpha, digits, I.ext(ell), MODS, LOGN, ST, str);
            } else {
                dev::ew_permute_sum_members(c0, qb, KK, (int)ell, cnt, b0 > 0, str.d, B, ln, 2 * ln, MODS, LOGN, ST);
                dev::ks_inner_multikey_sum_members(acc, eb, qb + ln, KK, cnt, have_acc || b0 > 0, (int)ell, I.P.K,
                                                   (int)I.P.nall(), I.P.alpha, digits, B, mb, I.ext(ell), MODS, LOGN,
                                                   ST, str);
            }
        }
        have_acc = true;
    }
    if (!have_acc) throw std::invalid_argument("linear_transform_ext: no giants");
    auto tm2 = I.alloc((size_t)B * 2 * ln * 8);
    u64 *t = static_cast<u64 *>(tm2->p);
    I.ks_moddown(acc, ell, 2 * B, t, c0m ? static_cast<const u64 *>(c0m->p) : nullptr, ln);
    auto r = new_ct(x.level + 1, x.slots, I.P.delta[x.level + 1], ell - 1, B);
    I.rescale(t, ell, ln, 2 * B, r->data);
    ctr.keyswitch += (keyed + (size_t)S) * B;
    ctr.rotations += (keyed + (size_t)S) * B;
    ctr.ptmult += npt * B;
    ctr.rescale += B;
    count_bytes((4.0 * ell + ks_units(ell)) * (double)(keyed + (size_t)S) + 3.0 * ell * (double)npt, B);
    return r;
}

CtPtr Engine::mod_raise(const Ciphertext &a) {
    auto &I = *impl;
    if (a.limbs != 1) throw std::invalid_argument("mod_raise: input must be at the last level (one limb)");
    const size_t nn = n(), nq = I.P.nq();
    const int segs = 2 * a.batch;
    auto cm = I.alloc((size_t)segs * nn * 8);
    u64 *c = static_cast<u64 *>(cm->p);
    dev::ntt_inverse_from(c, a.data, nn, 1, segs, nn, nullptr, I.T, ST);
    auto r = new_ct(0, a.slots, I.P.delta[0], nq, a.batch);
    dev::ew_lift_centered(r->data, c, 0, (int)nq, segs, nn, nq * nn, MODS, LOGN, ST);
    dev::ntt_forward(r->data, (int)nq, segs, nq * nn, nullptr, I.T, ST);
    count_bytes(2.0 + 2.0 * nq, a.batch);
    return r;
}

CtPtr Engine::linear_sum_to(const std::vector<const Ciphertext *> &xs, const std::vector<double> &c, int target) {
    auto &I = *impl;
    if (target > I.P.L) throw std::runtime_error("linear_sum_to: no levels left");
    if (xs.empty()) throw std::invalid_argument("linear_sum_to: no inputs");
    const int B = xs[0]->batch;
    const int segs = 2 * B;
    const size_t nn = n(), ell = I.P.limbs_at(target - 1);
    const double qd = (double)I.P.primes[I.P.L - target + 1];
    count_bytes(2.0 * ell * xs.size() + 2.0 * ell, B);
    auto tm = I.alloc((size_t)segs * ell * nn * 8);
    u64 *t = static_cast<u64 *>(tm->p);
    // group inputs by their limb count (segment stride) so each launch has one xseg
    std::map<size_t, std::vector<size_t>> by_limbs;
    for (size_t i = 0; i < xs.size(); ++i) {
        if (xs[i]->level > target - 1) throw std::invalid_argument("linear_sum_to: input level too high");
        if (xs[i]->batch != B) throw std::invalid_argument("linear_sum_to: batch size mismatch");
        by_limbs[xs[i]->limbs].push_back(i);
    }
    ctr.constmult += xs.size() * B;
    bool first = true;
    for (auto &kv : by_limbs) {
        std::vector<const u64 *> p;
        std::vector<int64_t> k;
        std::vector<uint8_t> sh;
        for (size_t i : kv.second) {
            const host::SConst K = host::const_to_target(c[i], I.P.delta[target], (u64)qd, xs[i]->scale);
            p.push_back(xs[i]->data);
            k.push_back(K.k);
            sh.push_back((uint8_t)K.sh);
        }
        // accumulate: first group writes, later groups add
        if (first) {
            dev::ew_linear_sum(t, p.data(), k.data(), (int)p.size(), (int)ell, segs, ell * nn, kv.first * nn, MODS,
                               LOGN, ST, false, sh.data());
            first = false;
        } else {
            auto sm = I.alloc((size_t)segs * ell * nn * 8);
            u64 *s = static_cast<u64 *>(sm->p);
            dev::ew_linear_sum(s, p.data(), k.data(), (int)p.size(), (int)ell, segs, ell * nn, kv.first * nn, MODS,
                               LOGN, ST, false, sh.data());
            dev::ew_add(t, t, s, (int)ell, segs, seg3(ell * nn, ell * nn, ell * nn), MODS, LOGN, ST);
        }
    }
    ctr.rescale += B;
    auto r = new_ct(target, xs[0]->slots, I.P.delta[target], ell - 1, B);
    I.rescale(t, ell, ell * nn, segs, r->data);
    return r;
}

// Several linear sums of the same inputs to one target level: row g of `c`
// gives the coefficients of output g.  Equal, word for word, to one
// linear_sum_to per row, but each input is streamed once per pass of up to
// 10 outputs.
// consts (rescaled sums only): output g is add_const(sum_g, (*consts)[g]) word
// for word.  The rescale is linear in c0 and divides by q_last, so the sum
// kernel adds K_g q_last mod q_l, K_g = const_at_scale(c, delta[target]), to c0
// on the limbs below the last (the last limb, all the rescale reads of it, stays
// what it was) and the rescale stores add_const's canonical words: no pass and
// no copy per output (mul_add's out_const does the same in the tensor pass).
std::vector<CtPtr> Engine::linear_sums_to(const std::vector<const Ciphertext *> &xs,
                                          const std::vector<std::vector<double>> &c, int target, bool rescale,
                                          const std::vector<double> *consts) {
    auto &I = *impl;
    if (target > I.P.L) throw std::runtime_error("linear_sums_to: no levels left");
    if (xs.empty()) throw std::invalid_argument("linear_sums_to: no inputs");
    if (consts && !rescale) throw std::invalid_argument("linear_sums_to: constants go with rescaled sums only");
    if (consts && consts->size() != c.size()) throw std::invalid_argument("linear_sums_to: one constant per output");
    const int B = xs[0]->batch;
    const size_t ell = I.P.limbs_at(target - 1), m = xs.size(), G = c.size();
    const u64 qd = I.P.primes[I.P.L - target + 1];
    count_bytes((2.0 * ell * m + 2.0 * ell) * G, B);  // op model: one linear sum per output
    // the doubles as (K, sh) pairs: K 2^sh at the scale each input needs to reach the target's
    std::vector<int64_t> K(G * m), Kc(consts ? G : 0);
    std::vector<uint8_t> sh(G * m), shc(consts ? G : 0);
    for (size_t g = 0; g < G && consts; ++g) {
        const double cg = (*consts)[g];
        const host::SConst k = cg != 0.0 ? host::const_at_scale(cg, I.P.delta[target]) : host::SConst{};
        Kc[g] = k.k;
        shc[g] = (uint8_t)k.sh;
        if (cg != 0.0) count_bytes(4.0 * (ell - 1), B);  // the add_const copy it replaces
    }
    for (size_t g = 0; g < G; ++g) {
        if (c[g].size() != m) throw std::invalid_argument("linear_sums_to: coefficient row size");
        for (size_t i = 0; i < m; ++i) {
            const host::SConst k = host::const_to_target(c[g][i], I.P.delta[target], qd, xs[i]->scale);
            K[g * m + i] = k.k;
            sh[g * m + i] = (uint8_t)k.sh;
        }
    }
    return linear_sums_run(xs, K.data(), sh.data(), consts ? Kc.data() : nullptr, consts ? shc.data() : nullptr, G,
                           target, rescale, "linear_sums_to");
}

std::vector<CtPtr> Engine::linear_sums_raw(const std::vector<const Ciphertext *> &xs, const int64_t *K,
                                           const uint8_t *sh, size_t G, const int64_t *Kc, const uint8_t *shc,
                                           int level) {
    auto &I = *impl;
    if (level < 0 || level >= I.P.L) throw std::invalid_argument("linear_sums_raw: level out of range");
    if (xs.empty() || G == 0) throw std::invalid_argument("linear_sums_raw: no inputs or no outputs");
    if (!K || !sh || (Kc && !shc)) throw std::invalid_argument("linear_sums_raw: null table");
    const int64_t lim = (int64_t)1 << 62;
    for (size_t t = 0; t < G * xs.size(); ++t)
        if (K[t] > lim || K[t] < -lim) throw std::invalid_argument("linear_sums_raw: |K| above 2^62");
    for (size_t g = 0; g < G && Kc; ++g)
        if (Kc[g] > lim || Kc[g] < -lim) throw std::invalid_argument("linear_sums_raw: |K| above 2^62");
    return linear_sums_run(xs, K, sh, Kc, shc, G, level + 1, false, "linear_sums_raw");
}

// linear_sums_to behind the doubles: K, sh [G][m], Kc, shc [G] or null
std::vector<CtPtr> Engine::linear_sums_run(const std::vector<const Ciphertext *> &xs, const int64_t *Kall,
                                           const uint8_t *shall, const int64_t *Kc, const uint8_t *shc, size_t Gall,
                                           int target, bool rescale, const char *who) {
    auto &I = *impl;
    const int B = xs[0]->batch, segs = 2 * B;
    const size_t nn = n(), ell = I.P.limbs_at(target - 1), m = xs.size();
    const u64 qd = I.P.primes[I.P.L - target + 1];
    std::vector<const u64 *> xp(m);
    std::vector<size_t> xseg(m);
    for (size_t i = 0; i < m; ++i) {
        if (xs[i]->level > target - 1) throw std::invalid_argument(std::string(who) + ": input level too high");
        if (xs[i]->batch != B) throw std::invalid_argument(std::string(who) + ": batch size mismatch");
        xp[i] = xs[i]->data;
        xseg[i] = xs[i]->limbs * nn;
    }
    std::vector<CtPtr> outs;
    // passes of at most LEAF_G = 32 outputs (the kernel's limit), balanced: 36 -> 18 + 18
    const size_t passes = (Gall + dev::LEAF_G - 1) / dev::LEAF_G, per = (Gall + passes - 1) / passes;
    const bool mfma = dev::linear_sums_on_mfma(LOGN) && m <= (size_t)dev::LEAF_M;
    for (size_t g0 = 0; g0 < Gall; g0 += per) {
        const int G = (int)std::min<size_t>(per, Gall - g0);
        // (with constants: G more entries behind the [G][m] rows, ew_linear_sum_multi's cfold)
        std::vector<int64_t> K(Kall + g0 * m, Kall + (g0 + G) * m);
        std::vector<uint8_t> sh(shall + g0 * m, shall + (g0 + G) * m);
        if (Kc) {
            K.insert(K.end(), Kc + g0, Kc + g0 + G);
            sh.insert(sh.end(), shc + g0, shc + g0 + G);
        }
        auto tm = I.alloc((size_t)G * segs * ell * nn * 8);
        u64 *t = static_cast<u64 *>(tm->p);
        std::vector<u64 *> op(G);
        for (int g = 0; g < G; ++g) op[g] = t + (size_t)g * segs * ell * nn;
        std::pair<const int64_t *, const uint8_t *> dk{nullptr, nullptr};
        if (mfma) dk = I.const_table(K, sh);
        dev::ew_linear_sum_multi(op.data(), G, xp.data(), xseg.data(), K.data(), (int)m, (int)ell, segs, ell * nn,
                                 MODS, LOGN, ST, sh.data(), dk.first, dk.second, Kc ? (int)ell - 1 : 0, qd);
        if (!rescale) {  // raw sums at the pre-rescale scale, views into one allocation
            for (int g = 0; g < G; ++g) {
                auto r = std::make_shared<Ciphertext>();
                r->mem = tm;
                r->data = op[g];
                r->level = target - 1;
                r->slots = xs[0]->slots;
                r->scale = I.P.delta[target] * (double)qd;
                r->limbs = ell;
                r->batch = B;
                outs.push_back(r);
            }
            ctr.constmult += (u64)G * m * B;
            continue;
        }
        auto rm = I.alloc((size_t)G * segs * (ell - 1) * nn * 8);  // all G outputs rescaled in one pass
        I.rescale(t, ell, ell * nn, G * segs, static_cast<u64 *>(rm->p));
        for (int g = 0; g < G; ++g) {
            auto r = std::make_shared<Ciphertext>();
            r->mem = rm;
            r->data = static_cast<u64 *>(rm->p) + (size_t)g * segs * (ell - 1) * nn;
            r->level = target;
            r->slots = xs[0]->slots;
            r->scale = I.P.delta[target];
            r->limbs = ell - 1;
            r->batch = B;
            outs.push_back(r);
        }
        ctr.constmult += (u64)G * m * B;
        ctr.rescale += (u64)G * B;
    }
    return outs;
}

CtPtr Engine::trivial_const(double c, int level, int slots, int batch) {
    auto r = zero_like(level, slots, batch);
    const host::SConst K = host::const_at_scale(c, impl->P.delta[level]);
    const size_t l2 = 2 * r->limbs * n();
    dev::ew_add_scalar(r->data, r->data, K.k, (int)r->limbs, batch, seg3(l2, l2, 0), MODS, LOGN, ST, K.sh);
    return r;
}
CtPtr Engine::zero_like(int level, int slots, int batch) {
    const size_t ell = impl->P.limbs_at(level);
    auto r = new_ct(level, slots, impl->P.delta[level], ell, batch);
    HIP_OK(hipMemsetAsync(r->data, 0, 2 * (size_t)batch * ell * n() * 8, ST));
    return r;
}
void Engine::reduce_after_allreduce(Ciphertext &ct) {
    dev::ew_reduce(ct.data, (int)ct.limbs, 2 * ct.batch, ct.limbs * n(), MODS, LOGN, ST);
}

// ---------------------------------------------------------------- batches --
CtPtr Engine::stack(const std::vector<const Ciphertext *> &xs) {
    if (xs.empty()) throw std::invalid_argument("stack: no inputs");
    int B = 0;
    for (auto *x : xs) {
        if (x->level != xs[0]->level) throw std::invalid_argument("stack: level mismatch");
        B += x->batch;
    }
    auto r = new_ct(xs[0]->level, xs[0]->slots, xs[0]->scale, xs[0]->limbs, B);
    const size_t ct_words = 2 * xs[0]->limbs * n();
    size_t off = 0;
    for (auto *x : xs) {
        HIP_OK(hipMemcpyAsync(r->data + off, x->data, x->batch * ct_words * 8, hipMemcpyDeviceToDevice, ST));
        off += x->batch * ct_words;
    }
    return r;
}
CtPtr Engine::member(const Ciphertext &a, int m) {
    if (m < 0 || m >= a.batch) throw std::out_of_range("member: index out of range");
    auto r = std::make_shared<Ciphertext>(a);
    r->data = a.data + (size_t)m * 2 * a.limbs * n();
    r->batch = 1;
    return r;
}
CtPtr Engine::sub_stacked(const Ciphertext &a0, const std::vector<const Ciphertext *> &bs) {
    if (bs.empty()) throw std::invalid_argument("sub_stacked: no operands");
    if (a0.batch != 1) throw std::invalid_argument("sub_stacked: a must be one ciphertext");
    const int level = bs[0]->level;
    for (auto *b : bs)
        if (b->level != level || b->batch != 1) throw std::invalid_argument("sub_stacked: operands differ in level");
    CtPtr a = std::make_shared<Ciphertext>(a0);
    if (a->level < level) a = level_adjust(*a, level);  // sub(a, b) adjusts a the same way
    if (a->level > level) {                             // ... or every b: not stackable in place
        std::vector<CtPtr> d;
        std::vector<const Ciphertext *> p;
        for (auto *b : bs) {
            d.push_back(sub(a0, *b));
            p.push_back(d.back().get());
        }
        return stack(p);
    }
    const size_t ln = a->limbs * n();
    auto r = new_ct(a->level, a->slots, a->scale, a->limbs, (int)bs.size());
    for (size_t i = 0; i < bs.size(); ++i)
        dev::ew_sub(r->data + i * 2 * ln, a->data, bs[i]->data, (int)a->limbs, 2, seg3(ln, ln, ln), MODS, LOGN, ST);
    count_bytes(6.0 * a->limbs, (int)bs.size());
    return r;
}
// FHE_TIEBREAK_FUSED (A/B, default 1): sub_add_plain_stacked's one-pass kernel
static bool tiebreak_fused_enabled() {
    static const bool on = env_switch("FHE_TIEBREAK_FUSED", 1);
    return on;
}
CtPtr Engine::sub_add_plain_stacked(const Ciphertext &a0, const std::vector<const Ciphertext *> &bs,
                                    const std::vector<const Plaintext *> &ps) {
    if (bs.empty()) throw std::invalid_argument("sub_add_plain_stacked: no operands");
    if (ps.size() != bs.size()) throw std::invalid_argument("sub_add_plain_stacked: one plaintext per operand");
    if (a0.batch != 1) throw std::invalid_argument("sub_add_plain_stacked: a must be one ciphertext");
    for (auto *b : bs)
        if (!b || b->level != bs[0]->level || b->batch != 1)
            throw std::invalid_argument("sub_add_plain_stacked: operands differ in level");
    // the plaintexts meet the differences, which sit at the deeper of the two levels
    const int level = std::max(a0.level, bs[0]->level);
    for (auto *p : ps)
        if (!p || p->level != level) throw std::invalid_argument("sub_add_plain_stacked: level mismatch");
    if (a0.level > bs[0]->level) {  // every b is adjusted instead: per-member ops, as sub_stacked
        std::vector<CtPtr> d;
        std::vector<const Ciphertext *> v;
        for (size_t i = 0; i < bs.size(); ++i) {
            d.push_back(add_plain(*sub(a0, *bs[i]), *ps[i]));
            v.push_back(d.back().get());
        }
        return stack(v);
    }
    const size_t nn = n();
    if (!tiebreak_fused_enabled()) {  // the plain form (A/B): the stacked differences, then c0 += p_i in place
        CtPtr r = sub_stacked(a0, bs);
        const size_t ln = r->limbs * nn;
        for (size_t i = 0; i < ps.size(); ++i) {
            u64 *c0 = r->data + i * 2 * ln;
            dev::ew_add(c0, c0, ps[i]->data, (int)r->limbs, 1, seg3(ln, ln, ln), MODS, LOGN, ST);
        }
        count_bytes(3.0 * r->limbs, (int)ps.size());
        return r;
    }
    CtPtr a = std::make_shared<Ciphertext>(a0);
    if (a->level < level) a = level_adjust(*a, level);  // sub(a, b) adjusts a the same way
    const size_t ell = a->limbs;
    const int B = (int)bs.size();
    auto r = new_ct(a->level, a->slots, a->scale, ell, B);
    std::vector<const u64 *> bp, pp;
    for (int i = 0; i < B; ++i) {
        if (bs[i]->limbs != ell || ps[i]->limbs != ell)  // the kernel reads ell limbs of each
            throw std::invalid_argument("sub_add_plain_stacked: operand limb count differs from its level's");
        bp.push_back(bs[i]->data);
        pp.push_back(ps[i]->data);
    }
    dev::ew_sub_add_plain_stacked(r->data, a->data, bp.data(), pp.data(), B, (int)ell, MODS, LOGN, ST);
    const int tile = dev::SUB_TILE;
    count_bytes(5.0 * ell * B + 2.0 * ell * ((B + tile - 1) / tile), 1);
    return r;
}
CtPtr Engine::sub_pm_const_stacked(const Ciphertext &a0, const std::vector<const Ciphertext *> &bs, double c) {
    if (bs.empty()) throw std::invalid_argument("sub_pm_const_stacked: no operands");
    if (a0.batch != 1) throw std::invalid_argument("sub_pm_const_stacked: a must be one ciphertext");
    for (auto *b : bs)
        if (!b || b->level != bs[0]->level || b->batch != 1)
            throw std::invalid_argument("sub_pm_const_stacked: operands differ in level");
    const int B = (int)bs.size();
    if (a0.level > bs[0]->level) {  // every b is adjusted instead: per-member ops, as sub_stacked
        std::vector<CtPtr> d(2 * (size_t)B);
        std::vector<const Ciphertext *> v;
        for (int i = 0; i < B; ++i) {
            CtPtr di = sub(a0, *bs[i]);
            d[i] = add_const(*di, c);
            d[B + i] = add_const(*negate(*di), c);
        }
        for (auto &x : d) v.push_back(x.get());
        return stack(v);
    }
    if (!group_fused_enabled()) {  // the plain form (A/B): the stacked differences, then the two sides on the stack
        CtPtr d = sub_stacked(a0, bs);
        CtPtr plus = add_const(*d, c), minus = add_const(*negate(*d), c);
        return stack({plus.get(), minus.get()});
    }
    CtPtr a = std::make_shared<Ciphertext>(a0);
    if (a->level < bs[0]->level) a = level_adjust(*a, bs[0]->level);  // sub(a, b) adjusts a the same way
    const size_t ell = a->limbs;
    auto r = new_ct(a->level, a->slots, a->scale, ell, 2 * B);
    std::vector<const u64 *> bp;
    for (auto *b : bs) {
        if (b->limbs != ell)  // the kernel reads ell limbs of each
            throw std::invalid_argument("sub_pm_const_stacked: operand limb count differs from its level's");
        bp.push_back(b->data);
    }
    const host::SConst K = host::const_at_scale(c, a->scale);
    dev::ew_sub_pm_const_stacked(r->data, a->data, bp.data(), B, K.k, K.sh, (int)ell, MODS, LOGN, ST);
    const int tile = dev::SUB_TILE;
    count_bytes(6.0 * ell * B + 2.0 * ell * ((B + tile - 1) / tile), 1);
    return r;
}
// FHE_GATHER_FUSED (A/B, default 1): the one-pass kernels of sub_offsets_stacked and mul_gather
static bool gather_fused_enabled() {
    static const bool on = env_switch("FHE_GATHER_FUSED", 1);
    return on;
}
CtPtr Engine::sub_offsets_stacked(const Ciphertext &a0, const std::vector<const Ciphertext *> &bs,
                                  const std::vector<int> &offsets) {
    if (bs.empty()) throw std::invalid_argument("sub_offsets_stacked: no operands");
    if (offsets.empty()) throw std::invalid_argument("sub_offsets_stacked: no offsets");
    if (a0.batch != 1) throw std::invalid_argument("sub_offsets_stacked: a must be one ciphertext");
    for (auto *b : bs)
        if (!b || b->level != bs[0]->level || b->batch != 1)
            throw std::invalid_argument("sub_offsets_stacked: operands differ in level");
    const int B = (int)bs.size(), K = (int)offsets.size();
    auto oriented = [&](const Ciphertext &d, int o) {  // d + o, negated for o < 0
        CtPtr v = add_const(d, (double)o);
        return o < 0 ? negate(*v) : v;
    };
    if (a0.level > bs[0]->level) {  // every b is adjusted instead: per-member ops, as sub_stacked
        std::vector<CtPtr> d((size_t)K * B);
        std::vector<const Ciphertext *> v;
        for (int i = 0; i < B; ++i) {
            CtPtr di = sub(a0, *bs[i]);
            for (int k = 0; k < K; ++k) d[(size_t)k * B + i] = oriented(*di, offsets[k]);
        }
        for (auto &x : d) v.push_back(x.get());
        return stack(v);
    }
    if (!gather_fused_enabled()) {  // the plain form (A/B): the stacked differences, then every offset on the stack
        CtPtr d = sub_stacked(a0, bs);
        if (K == 1) return oriented(*d, offsets[0]);
        std::vector<CtPtr> parts;
        std::vector<const Ciphertext *> v;
        for (int k = 0; k < K; ++k) {
            parts.push_back(oriented(*d, offsets[k]));
            v.push_back(parts.back().get());
        }
        return stack(v);
    }
    CtPtr a = std::make_shared<Ciphertext>(a0);
    if (a->level < bs[0]->level) a = level_adjust(*a, bs[0]->level);  // sub(a, b) adjusts a the same way
    const size_t ell = a->limbs;
    auto r = new_ct(a->level, a->slots, a->scale, ell, K * B);
    std::vector<const u64 *> bp;
    for (auto *b : bs) {
        if (b->limbs != ell)  // the kernel reads ell limbs of each
            throw std::invalid_argument("sub_offsets_stacked: operand limb count differs from its level's");
        bp.push_back(b->data);
    }
    std::vector<int64_t> Ks(K);
    std::vector<int> shs(K);
    std::vector<uint8_t> negs(K);
    for (int k = 0; k < K; ++k) {
        const host::SConst C = host::const_at_scale((double)offsets[k], a->scale);
        Ks[k] = C.k;
        shs[k] = C.sh;
        negs[k] = offsets[k] < 0;
    }
    dev::ew_sub_offsets_stacked(r->data, a->data, bp.data(), B, Ks.data(), shs.data(), negs.data(), K, (int)ell, MODS,
                                LOGN, ST);
    const int tile = dev::SUB_TILE;
    count_bytes((2.0 * K + 2.0) * ell * B + 2.0 * ell * ((B + tile - 1) / tile), 1);
    return r;
}
CtPtr Engine::mul_gather(const Ciphertext &a, const Ciphertext &b, int Pn, int Kn) {
    if (Pn < 1) throw std::invalid_argument("mul_gather: no columns");
    if (Kn < 1) throw std::invalid_argument("mul_gather: no offsets");
    if (a.batch < 1 || a.batch % Kn != 0)
        throw std::invalid_argument("mul_gather: a holds " + std::to_string(a.batch) + " members, not a multiple of " +
                                    std::to_string(Kn) + " offsets");
    const int B = a.batch / Kn;
    if ((long long)b.batch != (long long)Pn * B)
        throw std::invalid_argument("mul_gather: b holds " + std::to_string(b.batch) + " members, need " +
                                    std::to_string(Pn) + " columns of " + std::to_string(B));
    if (b.level != a.level || b.limbs != a.limbs) throw std::invalid_argument("mul_gather: b is not at a's level");
    const int PKB = Pn * Kn * B;
    const size_t nn = n(), ell = a.limbs;
    if (!gather_fused_enabled()) {  // the plain form (A/B): one stacked mul per (column, offset), stacked
        std::vector<CtPtr> prod;
        std::vector<const Ciphertext *> v;
        for (int p = 0; p < Pn; ++p)
            for (int k = 0; k < Kn; ++k) {
                Ciphertext col = b, ser = a;
                col.data = b.data + (size_t)p * B * 2 * ell * nn;
                ser.data = a.data + (size_t)k * B * 2 * ell * nn;
                col.batch = ser.batch = B;
                prod.push_back(mul(ser, col));
                v.push_back(prod.back().get());
            }
        return prod.size() == 1 ? prod[0] : stack(v);
    }
    return product_tail(a, PKB, [&](u64 *d01, u64 *d2) {
        count_bytes(5.0 * ell + ks_units(ell), PKB);
        const int per = dev::TENSOR_TILE;
        count_bytes(2.0 * ell * ((Kn + per - 1) / per), Pn * B);
        dev::ew_tensor_gather(d01, d2, a.data, b.data, Pn, Kn, (int)ell, B, MODS, LOGN, ST);
    });
}
// FHE_LEX_FUSED (A/B, default 1): the one-pass kernels of sub_lex_stacked and mul_lex
static bool lex_fused_enabled() {
    static const bool on = env_switch("FHE_LEX_FUSED", 1);
    return on;
}
CtPtr Engine::sub_lex_stacked(const std::vector<const Ciphertext *> &as, const std::vector<const Ciphertext *> &bs,
                              const std::vector<const Plaintext *> &ps, double eps) {
    const int L = (int)as.size();
    if (L < 2 || L > 4) throw std::invalid_argument("sub_lex_stacked: 2 to 4 keys");
    if (bs.empty() || bs.size() % (size_t)L) throw std::invalid_argument("sub_lex_stacked: one operand list per key");
    const int B = (int)(bs.size() / (size_t)L);
    if (!ps.empty() && (int)ps.size() != B) throw std::invalid_argument("sub_lex_stacked: one plaintext per operand");
    for (auto *a : as)
        if (!a || a->batch != 1 || a->level != as[0]->level || a->limbs != as[0]->limbs)
            throw std::invalid_argument("sub_lex_stacked: the keys must be single ciphertexts at one level");
    for (auto *b : bs)
        if (!b || b->batch != 1 || b->level != bs[0]->level)
            throw std::invalid_argument("sub_lex_stacked: operands differ in level");
    // the plaintexts meet the differences, which sit at the deeper of the two levels
    const int level = std::max(as[0]->level, bs[0]->level);
    for (auto *p : ps)
        if (!p || p->level != level) throw std::invalid_argument("sub_lex_stacked: level mismatch");
    const bool above = as[0]->level > bs[0]->level;  // every b would be adjusted: per-member ops, as sub_stacked
    if (above || !lex_fused_enabled()) {
        std::vector<CtPtr> keep;
        std::vector<const Ciphertext *> v;
        for (int l = 0; l < L; ++l) {
            const std::vector<const Ciphertext *> bl(bs.begin() + (size_t)l * B, bs.begin() + (size_t)(l + 1) * B);
            if (above) {
                std::vector<CtPtr> d;
                for (auto *b : bl) d.push_back(sub(*as[l], *b));
                if (l < L - 1) {
                    for (auto &x : d) keep.push_back(add_const(*x, eps));
                    for (auto &x : d) keep.push_back(add_const(*x, -eps));
                } else {
                    for (int i = 0; i < B; ++i) keep.push_back(ps.empty() ? d[i] : add_plain(*d[i], *ps[i]));
                }
            } else if (l < L - 1) {  // the plain form (A/B): the stacked differences, then the two sides on the stack
                CtPtr d = sub_stacked(*as[l], bl);
                keep.push_back(add_const(*d, eps));
                keep.push_back(add_const(*d, -eps));
            } else {
                keep.push_back(ps.empty() ? sub_stacked(*as[l], bl) : sub_add_plain_stacked(*as[l], bl, ps));
            }
        }
        for (auto &x : keep) v.push_back(x.get());
        return stack(v);
    }
    std::vector<CtPtr> adj;  // sub(a, b) adjusts a the same way
    std::vector<const u64 *> ap, bp, pp;
    for (auto *a : as) {
        if (a->level < level) {
            adj.push_back(level_adjust(*a, level));
            a = adj.back().get();
        }
        ap.push_back(a->data);
    }
    const Ciphertext &a0 = adj.empty() ? *as[0] : *adj[0];
    const size_t ell = a0.limbs;
    for (auto *b : bs) {
        if (b->limbs != ell)  // the kernel reads ell limbs of each
            throw std::invalid_argument("sub_lex_stacked: operand limb count differs from its level's");
        bp.push_back(b->data);
    }
    for (auto *p : ps) {
        if (p->limbs != ell) throw std::invalid_argument("sub_lex_stacked: plaintext limb count differs from its level's");
        pp.push_back(p->data);
    }
    auto r = new_ct(a0.level, a0.slots, a0.scale, ell, (2 * L - 1) * B);
    const host::SConst Kp = host::const_at_scale(eps, a0.scale), Kn = host::const_at_scale(-eps, a0.scale);
    dev::ew_sub_lex_stacked(r->data, ap.data(), L, bp.data(), pp.empty() ? nullptr : pp.data(), B, Kp.k, Kp.sh, Kn.k,
                            Kn.sh, (int)ell, MODS, LOGN, ST);
    const int tile = dev::SUB_TILE;
    const double tiles = (double)((B + tile - 1) / tile);
    count_bytes((L - 1) * (6.0 * ell * B + 2.0 * ell * tiles) + (pp.empty() ? 4.0 : 5.0) * ell * B + 2.0 * ell * tiles, 1);
    return r;
}
CtPtr Engine::mul_lex(const Ciphertext &t, double t_const, const Ciphertext &u, const Ciphertext &w) {
    if (u.batch < 1 || w.batch != u.batch || t.batch != u.batch)
        throw std::invalid_argument("mul_lex: t, u and w differ in member count");
    if (w.level != u.level || w.limbs != u.limbs) throw std::invalid_argument("mul_lex: u and w differ in level");
    if (!lex_fused_enabled())  // the plain form (A/B): every step an op of its own
        return mul(t_const != 0.0 ? *add_const(t, t_const) : t, *sub(u, w));
    if (t.level != u.level || t.limbs != u.limbs)  // mul level-adjusts an operand: u - w first, then the product
        return mul_add(t, *sub(u, w), {}, {}, nullptr, nullptr, t_const, 0.0);
    const int B = t.batch;
    const size_t nn = n(), ell = t.limbs;
    return product_tail(t, B, [&](u64 *d01, u64 *d2) {
        // the product, the sub it replaces and, with a constant, add_const's copy
        count_bytes(6.0 * ell + ks_units(ell) + 6.0 * ell + (t_const != 0.0 ? 4.0 * ell : 0.0), B);
        const host::SConst Ka = t_const != 0.0 ? host::const_at_scale(t_const, t.scale) : host::SConst{};
        dev::ew_tensor_lex(d01, d2, t.data, u.data, w.data, (int)ell, B, 2 * ell * nn, Ka.k, Ka.sh, MODS, LOGN, ST);
    });
}
// FHE_RUN_FUSED (A/B, default 1): the one-pass kernels of sub_bounds_stacked and mul_pairs_const / mul_pairs_sub
static bool run_fused_enabled() {
    static const bool on = env_switch("FHE_RUN_FUSED", 1);
    return on;
}
CtPtr Engine::sub_bounds_stacked(const std::vector<const Ciphertext *> &as, const std::vector<const Ciphertext *> &bs,
                                 const std::vector<double> &consts) {
    const int V = (int)as.size();
    if (V < 1 || V > 2) throw std::invalid_argument("sub_bounds_stacked: 1 or 2 left operands");
    if ((int)consts.size() != V) throw std::invalid_argument("sub_bounds_stacked: one constant per left operand");
    if (bs.empty()) throw std::invalid_argument("sub_bounds_stacked: no operands");
    for (auto *a : as)
        if (!a || a->batch != 1 || a->level != as[0]->level || a->limbs != as[0]->limbs || a->slots != as[0]->slots)
            throw std::invalid_argument("sub_bounds_stacked: the left operands must be single ciphertexts at one level");
    for (auto *b : bs)
        if (!b || b->level != bs[0]->level || b->batch != 1)
            throw std::invalid_argument("sub_bounds_stacked: operands differ in level");
    const int B = (int)bs.size();
    const bool above = as[0]->level > bs[0]->level;  // every b would be adjusted: per-member ops, as sub_stacked
    if (above || !run_fused_enabled()) {
        std::vector<CtPtr> keep;
        std::vector<const Ciphertext *> v;
        for (int k = 0; k < V; ++k) {
            if (above) {
                for (auto *b : bs) keep.push_back(add_const(*sub(*as[k], *b), consts[k]));
            } else {  // the plain form (A/B): the stacked differences, then the constant on the stack in place
                CtPtr d = sub_stacked(*as[k], bs);
                add_const_inplace(d, consts[k]);
                keep.push_back(d);
            }
        }
        if (keep.size() == 1) return keep[0];
        for (auto &x : keep) v.push_back(x.get());
        return stack(v);
    }
    const int level = bs[0]->level;
    std::vector<CtPtr> adj;  // sub(a, b) adjusts a the same way
    std::vector<const u64 *> ap, bp;
    for (auto *a : as) {
        if (a->level < level) {
            adj.push_back(level_adjust(*a, level));
            a = adj.back().get();
        }
        ap.push_back(a->data);
    }
    const Ciphertext &a0 = adj.empty() ? *as[0] : *adj[0];
    const size_t ell = a0.limbs;
    for (auto *b : bs) {
        if (b->limbs != ell)  // the kernel reads ell limbs of each
            throw std::invalid_argument("sub_bounds_stacked: operand limb count differs from its level's");
        bp.push_back(b->data);
    }
    auto r = new_ct(a0.level, a0.slots, a0.scale, ell, V * B);
    int64_t Ks[2] = {0, 0};
    int shs[2] = {0, 0};
    for (int k = 0; k < V; ++k) {
        const host::SConst K = host::const_at_scale(consts[k], a0.scale);
        Ks[k] = K.k;
        shs[k] = K.sh;
    }
    dev::ew_sub_bounds_stacked(r->data, ap.data(), V, bp.data(), B, Ks, shs, (int)ell, MODS, LOGN, ST);
    const int tile = dev::SUB_TILE;
    count_bytes((2.0 + 2.0 * V) * ell * B + 2.0 * V * ell * ((B + tile - 1) / tile), 1);
    return r;
}
CtPtr Engine::mul_pairs_const(const Ciphertext &a, double c, const Ciphertext &b, int Pn) {
    return mul_pairs_left("mul_pairs_const", a, nullptr, c, b, Pn);
}
CtPtr Engine::mul_pairs_sub(const Ciphertext &a, const Ciphertext &a_sub, const Ciphertext &b, int Pn) {
    return mul_pairs_left("mul_pairs_sub", a, &a_sub, 0.0, b, Pn);
}
CtPtr Engine::mul_pairs_left(const char *what, const Ciphertext &a, const Ciphertext *w, double c, const Ciphertext &b,
                             int Pn) {
    const std::string me(what);
    if (Pn < 1) throw std::invalid_argument(me + ": no columns");
    if (a.batch < 1) throw std::invalid_argument(me + ": a holds no member");
    if (w && w->batch != a.batch) throw std::invalid_argument(me + ": a and a_sub differ in member count");
    if (w && (w->level != a.level || w->limbs != a.limbs)) throw std::invalid_argument(me + ": a and a_sub differ in level");
    if ((long long)b.batch != (long long)Pn * a.batch)
        throw std::invalid_argument(me + ": b holds " + std::to_string(b.batch) + " members, need " + std::to_string(Pn) +
                                    " columns of " + std::to_string(a.batch));
    if (b.level != a.level || b.limbs != a.limbs) throw std::invalid_argument(me + ": b is not at a's level");
    const int B = a.batch, PB = Pn * B;
    const size_t nn = n(), ell = a.limbs;
    if (!run_fused_enabled()) {  // the plain form (A/B): the left operand written out, then one mul per column, stacked
        CtPtr left = w ? sub(a, *w) : add_const(a, c);
        std::vector<CtPtr> prod;
        std::vector<const Ciphertext *> v;
        for (int p = 0; p < Pn; ++p) {
            Ciphertext col = b;
            col.data = b.data + (size_t)p * B * 2 * ell * nn;
            col.batch = B;
            prod.push_back(mul(*left, col));
            v.push_back(prod.back().get());
        }
        return prod.size() == 1 ? prod[0] : stack(v);
    }
    return product_tail(a, PB, [&](u64 *d01, u64 *d2) {
        count_bytes(5.0 * ell + ks_units(ell), PB);
        const int per = dev::TENSOR_TILE;
        count_bytes((w ? 4.0 : 2.0) * ell * ((Pn + per - 1) / per), B);
        const host::SConst K = w ? host::SConst{} : host::const_at_scale(c, a.scale);
        dev::ew_tensor_run(d01, d2, a.data, w ? w->data : nullptr, b.data, Pn, (int)ell, B, 2 * ell * nn, K.k, K.sh,
                           MODS, LOGN, ST);
    });
}
// FHE_WIN_FUSED (A/B, default 1): the one-pass kernels of sub_window_stacked and mul_sub_sub
static bool win_fused_enabled() {
    static const bool on = env_switch("FHE_WIN_FUSED", 1);
    return on;
}
CtPtr Engine::sub_window_stacked(const std::vector<const Ciphertext *> &part_as,
                                 const std::vector<const Ciphertext *> &part_bs, const Ciphertext *order_a,
                                 const Ciphertext *order_lo, const std::vector<const Ciphertext *> &order_bs,
                                 const std::vector<const Plaintext *> &ps, double order_const, double eps) {
    const int G = (int)part_as.size();
    if (G < 1 || G > 3) throw std::invalid_argument("sub_window_stacked: 1 to 3 partition keys");
    if (part_bs.empty() || part_bs.size() % (size_t)G)
        throw std::invalid_argument("sub_window_stacked: one operand list per partition key");
    const int B = (int)(part_bs.size() / (size_t)G);
    if (!order_a && (order_lo || !order_bs.empty() || !ps.empty()))
        throw std::invalid_argument("sub_window_stacked: order operands without an order key");
    if (order_a && (int)order_bs.size() != B)
        throw std::invalid_argument("sub_window_stacked: one order operand per partition operand");
    if (!ps.empty() && ((int)ps.size() != B || order_lo))
        throw std::invalid_argument("sub_window_stacked: one plaintext per operand, and none beside a lower bound");
    const int kind = !order_a ? 0 : order_lo ? 3 : !ps.empty() ? 2 : 1;
    std::vector<const Ciphertext *> as = part_as, bs = part_bs;
    if (order_a) {
        as.push_back(order_a);
        bs.insert(bs.end(), order_bs.begin(), order_bs.end());
    }
    if (order_lo) as.push_back(order_lo);
    for (auto *a : as)
        if (!a || a->batch != 1 || a->level != as[0]->level || a->limbs != as[0]->limbs || a->slots != as[0]->slots)
            throw std::invalid_argument("sub_window_stacked: the keys must be single ciphertexts at one level");
    for (auto *b : bs)
        if (!b || b->batch != 1 || b->level != bs[0]->level)
            throw std::invalid_argument("sub_window_stacked: operands differ in level");
    // the plaintexts meet the differences, which sit at the deeper of the two levels
    const int level = std::max(as[0]->level, bs[0]->level);
    for (auto *p : ps)
        if (!p || p->level != level) throw std::invalid_argument("sub_window_stacked: level mismatch");
    const bool above = as[0]->level > bs[0]->level;  // every b would be adjusted: per-member ops, as sub_stacked
    if (above || !win_fused_enabled()) {
        std::vector<CtPtr> keep;
        // member i of one side: add_const(sub(a, b_i), c); the plain form takes the stacked differences
        auto side = [&](const Ciphertext &a, const std::vector<const Ciphertext *> &bl, double c) {
            if (above) {
                for (auto *b : bl) keep.push_back(add_const(*sub(a, *b), c));
            } else {
                CtPtr d = sub_stacked(a, bl);
                add_const_inplace(d, c);
                keep.push_back(d);
            }
        };
        for (int g = 0; g < G; ++g) {
            const std::vector<const Ciphertext *> bl(part_bs.begin() + (size_t)g * B, part_bs.begin() + (size_t)(g + 1) * B);
            side(*part_as[g], bl, eps);
            side(*part_as[g], bl, -eps);
        }
        if (kind == 1) {
            side(*order_a, order_bs, order_const);
        } else if (kind == 2) {
            CtPtr d = above ? nullptr : sub_stacked(*order_a, order_bs);
            for (int i = 0; i < B; ++i)
                keep.push_back(add_plain(above ? *sub(*order_a, *order_bs[i]) : *member(*d, i), *ps[i]));
        } else if (kind == 3) {
            side(*order_a, order_bs, eps);
            side(*order_lo, order_bs, -eps);
        }
        std::vector<const Ciphertext *> v;
        for (auto &x : keep) v.push_back(x.get());
        return stack(v);
    }
    std::vector<CtPtr> adj;  // sub(a, b) adjusts a the same way
    std::vector<const u64 *> ap, bp, pp;
    for (auto *a : as) {
        if (a->level < level) {
            adj.push_back(level_adjust(*a, level));
            a = adj.back().get();
        }
        ap.push_back(a->data);
    }
    const Ciphertext &a0 = adj.empty() ? *as[0] : *adj[0];
    const size_t ell = a0.limbs;
    for (auto *b : bs) {
        if (b->limbs != ell)  // the kernel reads ell limbs of each
            throw std::invalid_argument("sub_window_stacked: operand limb count differs from its level's");
        bp.push_back(b->data);
    }
    for (auto *p : ps) {
        if (p->limbs != ell)
            throw std::invalid_argument("sub_window_stacked: plaintext limb count differs from its level's");
        pp.push_back(p->data);
    }
    const int V = kind == 0 ? 0 : kind == 3 ? 2 : 1;
    auto r = new_ct(a0.level, a0.slots, a0.scale, ell, (2 * G + V) * B);
    const host::SConst Kp = host::const_at_scale(eps, a0.scale), Kn = host::const_at_scale(-eps, a0.scale);
    const host::SConst Ko = kind == 1 ? host::const_at_scale(order_const, a0.scale) : host::SConst{};
    dev::ew_sub_window_stacked(r->data, ap.data(), G, kind == 3 ? ap[(size_t)G + 1] : nullptr, bp.data(),
                               pp.empty() ? nullptr : pp.data(), kind, B, Kp.k, Kp.sh, Kn.k, Kn.sh, Ko.k, Ko.sh, (int)ell,
                               MODS, LOGN, ST);
    const int tile = dev::SUB_TILE;
    const double tiles = (double)((B + tile - 1) / tile);
    const double order = kind == 0   ? 0.0
                         : kind == 3 ? 6.0 * ell * B + 4.0 * ell * tiles
                                     : (kind == 2 ? 5.0 : 4.0) * ell * B + 2.0 * ell * tiles;
    count_bytes(G * (6.0 * ell * B + 2.0 * ell * tiles) + order, 1);
    return r;
}
CtPtr Engine::mul_sub_sub(const Ciphertext &u, const Ciphertext &w, const Ciphertext &u2, const Ciphertext &w2) {
    if (u.batch < 1 || w.batch != u.batch || u2.batch != u.batch || w2.batch != u.batch)
        throw std::invalid_argument("mul_sub_sub: the operands differ in member count");
    if (w.level != u.level || w.limbs != u.limbs) throw std::invalid_argument("mul_sub_sub: u and w differ in level");
    if (w2.level != u2.level || w2.limbs != u2.limbs) throw std::invalid_argument("mul_sub_sub: u2 and w2 differ in level");
    // the plain form (A/B), and operands at two levels (mul level-adjusts one): every step an op of its own
    if (!win_fused_enabled() || u2.level != u.level || u2.limbs != u.limbs) return mul(*sub(u, w), *sub(u2, w2));
    const int B = u.batch;
    const size_t nn = n(), ell = u.limbs;
    return product_tail(u, B, [&](u64 *d01, u64 *d2) {
        count_bytes(11.0 * ell + ks_units(ell), B);
        dev::ew_tensor_win(d01, d2, u.data, w.data, u2.data, w2.data, (int)ell, B, 2 * ell * nn, MODS, LOGN, ST);
    });
}
CtPtr Engine::sub_plain_stacked(const Ciphertext &a, const std::vector<const Plaintext *> &ps) {
    if (ps.empty()) throw std::invalid_argument("sub_plain_stacked: no plaintexts");
    if (a.batch != 1) throw std::invalid_argument("sub_plain_stacked: a must be one ciphertext");
    for (auto *p : ps)
        if (p->level != a.level) throw std::invalid_argument("sub_plain_stacked: level mismatch");
    const size_t ln = a.limbs * n();
    auto r = new_ct(a.level, a.slots, a.scale, a.limbs, (int)ps.size());
    for (size_t i = 0; i < ps.size(); ++i)
        dev::ew_c0_op(r->data + i * 2 * ln, a.data, ps[i]->data, 0, 0, 2, (int)a.limbs, 1, MODS, LOGN, ST);
    count_bytes(5.0 * a.limbs, (int)ps.size());
    return r;
}
CtPtr Engine::sum_members(const Ciphertext &a) {
    auto r = new_ct(a.level, a.slots, a.scale, a.limbs, 1);
    dev::ew_sum_members(r->data, a.data, a.batch, (int)a.limbs, MODS, LOGN, ST);
    return r;
}
void Engine::sum_member_groups(const Ciphertext &a, int groups, CtPtr &acc) {
    if (groups < 1 || groups > 32767 || a.batch % groups)
        throw std::invalid_argument("sum_member_groups: the batch is not a whole number of groups");
    const int B = a.batch / groups;
    if (acc && (acc->batch != groups || acc->level != a.level || acc->limbs != a.limbs))
        throw std::invalid_argument("sum_member_groups: accumulator shape mismatch");
    if (!cols_fused_enabled()) {  // the plain form (A/B): one sum_members per group, stacked
        std::vector<CtPtr> sums;
        std::vector<const Ciphertext *> v;
        for (int p = 0; p < groups; ++p) {
            Ciphertext g = a;
            g.data = a.data + (size_t)p * B * 2 * a.limbs * n();
            g.batch = B;
            sums.push_back(sum_members(g));
            v.push_back(sums.back().get());
        }
        CtPtr r = groups == 1 ? sums[0] : stack(v);
        acc = acc ? add(*acc, *r) : r;
        return;
    }
    const bool inplace = acc && acc.use_count() == 1 && acc->mem && acc->mem.use_count() == 1;
    CtPtr r = inplace ? acc : new_ct(a.level, a.slots, a.scale, a.limbs, groups);
    dev::ew_sum_member_groups(r->data, a.data, groups, B, (int)a.limbs, inplace, MODS, LOGN, ST);
    count_bytes(2.0 * a.limbs * (B + 1) + (inplace ? 2.0 * a.limbs : 0.0), groups);
    if (acc && !inplace)
        acc = add(*acc, *r);
    else
        acc = r;
}

// =================================================== kernel-level (tests) ==
void Engine::ntt_host(u64 *data, int prime_index, int limbs, bool inverse) {
    auto &I = *impl;
    const size_t nn = n();
    auto m = I.alloc((size_t)limbs * nn * 8);
    u64 *d = static_cast<u64 *>(m->p);
    std::vector<int> pm(limbs);
    for (int i = 0; i < limbs; ++i) pm[i] = prime_index + i;
    auto pmm = I.alloc(limbs * sizeof(int));
    HIP_OK(hipMemcpyAsync(pmm->p, pm.data(), limbs * sizeof(int), hipMemcpyHostToDevice, ST));
    HIP_OK(hipMemcpyAsync(d, data, (size_t)limbs * nn * 8, hipMemcpyHostToDevice, ST));
    const int *pmd = static_cast<int *>(pmm->p);
    dev::ntt_register_map(pmd, pm.data(), pm.size());  // so the launch splits by prime class
    if (inverse)
        dev::ntt_inverse(d, limbs, 1, 0, pmd, I.T, ST);
    else
        dev::ntt_forward(d, limbs, 1, 0, pmd, I.T, ST);
    dev::ntt_unregister_map(pmd);
    HIP_OK(hipMemcpyAsync(data, d, (size_t)limbs * nn * 8, hipMemcpyDeviceToHost, ST));
    HIP_OK(hipStreamSynchronize(ST));
}
void Engine::modup_host(const u64 *d, size_t ell, u64 *ext) {
    auto &I = *impl;
    const size_t nn = n(), W = ell + I.P.K;
    const int digits = I.P.digits_at(ell);
    auto dm = I.alloc(ell * nn * 8);
    HIP_OK(hipMemcpyAsync(dm->p, d, ell * nn * 8, hipMemcpyHostToDevice, ST));
    auto e = I.modup(static_cast<u64 *>(dm->p), ell, 1, ell * nn);
    // own-digit limbs are not materialised on the device: fill them from d
    u64 *ep = static_cast<u64 *>(e->p);
    for (int j = 0; j < digits; ++j) {
        const size_t lo = (size_t)j * I.P.alpha, hi = std::min(ell, (size_t)(j + 1) * I.P.alpha);
        HIP_OK(hipMemcpyAsync(ep + ((size_t)j * W + lo) * nn, static_cast<u64 *>(dm->p) + lo * nn,
                              (hi - lo) * nn * 8, hipMemcpyDeviceToDevice, ST));
    }
    HIP_OK(hipMemcpyAsync(ext, ep, (size_t)digits * W * nn * 8, hipMemcpyDeviceToHost, ST));
    HIP_OK(hipStreamSynchronize(ST));
}
void Engine::moddown_host(const u64 *in, size_t ell, u64 *out) {
    auto &I = *impl;
    const size_t nn = n(), K = I.P.K, W = ell + K;
    auto im = I.alloc(W * nn * 8);
    u64 *x = static_cast<u64 *>(im->p);
    HIP_OK(hipMemcpyAsync(x, in, W * nn * 8, hipMemcpyHostToDevice, ST));
    dev::ntt_inverse(x + ell * nn, (int)K, 1, 0, I.ext(ell) + ell, I.T, ST, /*raw*/ true);
    auto cm = I.alloc(ell * nn * 8);
    u64 *conv = static_cast<u64 *>(cm->p);
    dev::moddown_convert(conv, x + ell * nn, (int)ell, (int)K, (int)I.P.nq(), W * nn, ell * nn, 1, I.phinv,
                         I.phinv_s, I.phat, I.pmod, I.pinvd, MODS, LOGN, ST);
    dev::ntt_forward(conv, (int)ell, 1, 0, nullptr, I.T, ST);
    auto om = I.alloc(ell * nn * 8);
    dev::moddown_finish(static_cast<u64 *>(om->p), x, conv, nullptr, (int)ell, 1, ell * nn, W * nn, 0, I.pinv,
                        I.pinv_s, MODS, LOGN, ST);
    HIP_OK(hipMemcpyAsync(out, om->p, ell * nn * 8, hipMemcpyDeviceToHost, ST));
    HIP_OK(hipStreamSynchronize(ST));
}
void Engine::ntt_dev(u64 *data, int prime_index, int limbs, int segments, size_t seg_stride, bool inverse,
                     void *stream) {
    auto &I = *impl;
    if (prime_index < 0 || limbs < 1 || segments < 1 || (size_t)(prime_index + limbs) > I.P.nall())
        throw std::invalid_argument("ntt_dev: primes [prime_index, prime_index + limbs) outside the context");
    if (segments > 1 && seg_stride < (size_t)limbs * n())
        throw std::invalid_argument("ntt_dev: segment stride shorter than a segment");
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : ST;
    const int *pm = prime_index == 0 ? nullptr : I.iota + prime_index;
    if (inverse)
        dev::ntt_inverse(data, limbs, segments, seg_stride, pm, I.T, st);
    else
        dev::ntt_forward(data, limbs, segments, seg_stride, pm, I.T, st);
}
void Engine::automorph_dev(const u64 *in, u64 *out, size_t limbs, u64 g, void *stream) {
    auto &I = *impl;
    if (g % 2 == 0 || g >= 2 * (u64)n()) throw std::invalid_argument("automorph_dev: galois element must be odd and < 2n");
    if (limbs < 1 || limbs > I.P.nall()) throw std::invalid_argument("automorph_dev: bad limb count");
    const uint32_t *pm = I.perm(g);  // built and uploaded on the engine stream, which perm() drains
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : ST;
    dev::ew_permute(out, in, pm, (int)limbs, 1, dev::Seg{0, 0, 0}, LOGN, st);
}
void Engine::automorph_host(const u64 *in, size_t limbs, u64 g, u64 *out) {
    auto &I = *impl;
    const size_t nn = n();
    auto im = I.alloc(limbs * nn * 8), om = I.alloc(limbs * nn * 8);
    HIP_OK(hipMemcpyAsync(im->p, in, limbs * nn * 8, hipMemcpyHostToDevice, ST));
    dev::ew_permute(static_cast<u64 *>(om->p), static_cast<u64 *>(im->p), I.perm(g), (int)limbs, 1, dev::Seg{0, 0, 0},
                    LOGN, ST);
    HIP_OK(hipMemcpyAsync(out, om->p, limbs * nn * 8, hipMemcpyDeviceToHost, ST));
    HIP_OK(hipStreamSynchronize(ST));
}

namespace {
struct EventClock final : dev::LaunchClock {
    struct Rec {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        const char *name = nullptr;
        const char *phase = nullptr;  // the launching thread's algorithm phase
        double bytes = 0;
    };
    std::map<std::string, double> phase_opbytes;  // op-level bytes per algorithm phase
    std::mutex mu;
    std::vector<Rec> recs;
    size_t used = 0;
    int events(hipEvent_t &start, hipEvent_t &stop) override {
        std::lock_guard<std::mutex> lk(mu);
        if (used == recs.size()) {
            Rec r;
            HIP_OK(hipEventCreate(&r.e0));
            HIP_OK(hipEventCreate(&r.e1));
            recs.push_back(r);
        }
        start = recs[used].e0;
        stop = recs[used].e1;
        return (int)used++;
    }
    void record(int slot, const char *kernel, double bytes) override {
        std::lock_guard<std::mutex> lk(mu);
        recs[(size_t)slot].name = kernel;
        recs[(size_t)slot].phase = dev::algo_phase();
        recs[(size_t)slot].bytes = bytes;
    }
    ~EventClock() override {
        for (auto &r : recs) {
            (void)hipEventDestroy(r.e0);
            (void)hipEventDestroy(r.e1);
        }
    }
};
std::unique_ptr<EventClock> g_clock;
}  // namespace

// live clock running: op-level bytes per algorithm phase (Engine::count_bytes)
void clock_phase_opbytes(const char *phase, u64 b) {
    if (!g_clock) return;
    std::lock_guard<std::mutex> lk(g_clock->mu);
    g_clock->phase_opbytes[phase] += (double)b;
}

void Engine::pool_trim() {  // this engine's pool and those of its forks (all pools of the process)
    HIP_OK(hipStreamSynchronize(impl->st));
    trim_all_pools();
}
void Engine::pool_stats(size_t &live, size_t &cached, size_t &peak) const {
    std::lock_guard<std::mutex> lk(impl->pool->mu);
    live = impl->pool->live;
    cached = impl->pool->cached;
    peak = impl->pool->peak;
}

const char *Engine::set_algo_phase(const char *phase) {
    const char *prev = dev::algo_phase();
    dev::algo_phase() = phase;
    return prev;
}

void Engine::kernel_clock_start() {
    if (dev::launch_clock()) throw std::runtime_error("kernel clock already running");
    g_clock = std::make_unique<EventClock>();
    dev::launch_clock() = g_clock.get();
}

std::string Engine::kernel_clock_stop() {
    if (!g_clock) throw std::runtime_error("kernel clock not running");
    dev::launch_clock() = nullptr;
    HIP_OK(hipDeviceSynchronize());  // lanes may have launched on their own streams
    struct Agg {
        long launches = 0;
        double ms = 0, bytes = 0;
    };
    std::map<std::string, Agg> agg;
    for (size_t i = 0; i < g_clock->used; ++i) {
        auto &r = g_clock->recs[i];
        float ms = 0;
        HIP_OK(hipEventElapsedTime(&ms, r.e0, r.e1));
        auto &a = agg[r.name];
        a.launches += 1;
        a.ms += ms;
        a.bytes += r.bytes;
        if (r.phase) {  // "phase:<name>": every clocked kernel of an algorithm phase
            auto &pa = agg[std::string("phase:") + r.phase];
            pa.launches += 1;
            pa.ms += ms;
            pa.bytes += r.bytes;
        }
    }
    std::map<std::string, double> phase_op = std::move(g_clock->phase_opbytes);
    g_clock.reset();
    std::string out = "{";
    char buf[512];
    bool first = true;
    for (auto &kv : agg) {
        const bool ph = kv.first.rfind("phase:", 0) == 0;
        const double op = ph ? phase_op[kv.first.substr(6)] : 0.0;
        snprintf(buf, sizeof buf, "%s\"%s\": {\"launches\": %ld, \"ms\": %.6f, \"bytes\": %.0f", first ? "" : ", ",
                 kv.first.c_str(), kv.second.launches, kv.second.ms, kv.second.bytes);
        out += buf;
        if (ph) {
            snprintf(buf, sizeof buf, ", \"op_bytes\": %.0f", op);
            out += buf;
        }
        out += "}";
        first = false;
    }
    return out + "}";
}

void Engine::time_kernel(const std::string &name, size_t ell, int iters, double &avg_ms, double &bytes) {
    auto &I = *impl;
    const size_t nn = n(), K = (size_t)I.P.K, W = ell + K, B = nn * 8;
    const int digits = I.P.digits_at(ell);
    if (ell < 1 || ell > I.P.nq()) throw std::invalid_argument("time_kernel: bad limb count");
    if (!I.ks->relin) throw std::runtime_error("time_kernel: needs the relinearisation key");
    // operands with random-looking contents (reduced residues)
    auto dm = I.alloc(3 * ell * nn * 8);
    auto em = I.alloc((size_t)digits * W * nn * 8);
    auto am = I.alloc(2 * W * nn * 8);
    u64 *d = static_cast<u64 *>(dm->p), *e = static_cast<u64 *>(em->p), *acc = static_cast<u64 *>(am->p);
    HIP_OK(hipMemsetAsync(d, 0x11, 3 * ell * nn * 8, ST));
    HIP_OK(hipMemsetAsync(e, 0x22, (size_t)digits * W * nn * 8, ST));
    dev::ew_reduce(d, (int)ell, 3, ell * nn, MODS, LOGN, ST);
    std::function<void()> launch;
    if (name == "ks_inner") {
        dev::KsStrides str;
        str.acc = 2 * W * nn;
        str.ext = (size_t)digits * W * nn;
        str.d = ell * nn;
        launch = [&, str] {
            dev::ks_inner(acc, e, d, static_cast<u64 *>(I.ks->relin->p), (int)ell, (int)K, (int)I.P.nq(), (int)I.P.nall(),
                          I.P.alpha, digits, nullptr, I.ext(ell), MODS, LOGN, ST, 1, str);
        };
        bytes = (double)((size_t)digits * W * 3 + 2 * W) * B;  // ext + key(b,a) read, 2 accumulators written
    } else if (name == "ntt_fwd") {
        launch = [&] { dev::ntt_forward(e, (int)W, digits, W * nn, I.ext(ell), I.T, ST); };
        bytes = 2.0 * 2.0 * (double)(W * digits) * B;  // two passes, each reads + writes every limb
    } else if (name == "ntt_inv_row32" || name == "ntt_fwd_row32") {  // 32 ciphertext members of ell limbs
        const bool fwd = name == "ntt_fwd_row32";
        auto bm = I.alloc((size_t)32 * ell * nn * 8);
        u64 *buf = static_cast<u64 *>(bm->p);
        HIP_OK(hipMemsetAsync(buf, 0x33, (size_t)32 * ell * nn * 8, ST));
        dev::ew_reduce(buf, (int)ell, 32, ell * nn, MODS, LOGN, ST);
        em = bm;  // keep alive
        launch = [&, buf, fwd] { dev::ntt_row_pass(buf, (int)ell, 32, ell * nn, nullptr, I.T, ST, fwd); };
        bytes = 2.0 * 32.0 * (double)ell * B;
    } else if (name == "ntt_inv" || name == "ntt_fwd_row" || name == "ntt_inv_row") {
        const bool row = name != "ntt_inv", fwd = name == "ntt_fwd_row";
        launch = [&, row, fwd] {
            if (row)
                dev::ntt_row_pass(e, (int)W, digits, W * nn, I.ext(ell), I.T, ST, fwd);
            else
                dev::ntt_inverse(e, (int)W, digits, W * nn, I.ext(ell), I.T, ST);
        };
        bytes = (row ? 2.0 : 4.0) * (double)(W * digits) * B;
    } else if (name == "moddown_rescale32") {  // the HMult tail's conversion over 32 members (64 segments)
        const int segs = 64;
        auto bm = I.alloc((size_t)segs * W * nn * 8), cm = I.alloc((size_t)segs * ell * nn * 8);
        u64 *a = static_cast<u64 *>(bm->p), *corr = static_cast<u64 *>(cm->p);
        HIP_OK(hipMemsetAsync(a, 0x33, (size_t)segs * W * nn * 8, ST));
        dev::ew_reduce(a, (int)W, segs, W * nn, MODS, LOGN, ST);  // residues below every limb's prime
        em = bm;  // keep alive
        dm = cm;
        launch = [&, a, corr] {
            dev::moddown_rescale_convert(corr, a, (int)ell, (int)K, (int)I.P.nq(), W * nn, (ell - 1) * nn, segs, I.phinv,
                                         I.phinv_s, I.phat, I.pinv, I.pinv_s, I.pmod, I.pinvd, I.T.ninv, I.T.ninv_s,
                                         MODS, LOGN, ST, I.pmod_s, I.mdfp_c, I.mdfp_q, I.LT.mdfp_mid);
        };
        bytes = (double)segs * (K + 1 + ell - 1) * B;
    } else if (name == "modup_convert") {
        launch = [&] {
            dev::modup_convert(e, d, (int)ell, (int)K, I.P.alpha, digits, 1, ell * nn, (size_t)digits * W * nn,
                               I.ext(ell), I.modup_tab, I.LT.modup_off[ell].data(), MODS, LOGN, ST, I.modup_fp,
                               I.LT.modup_fp_off[ell].data(), I.LT.modup_fp_mid);
        };
        bytes = (double)(ell + (size_t)digits * W - ell) * B;
    } else if (name == "modup32") {  // ModUp's conversion over 32 members
        const int mem = 32;
        auto cm = I.alloc((size_t)mem * ell * nn * 8), xm = I.alloc((size_t)mem * digits * W * nn * 8);
        u64 *c = static_cast<u64 *>(cm->p), *x = static_cast<u64 *>(xm->p);
        HIP_OK(hipMemsetAsync(c, 0x44, (size_t)mem * ell * nn * 8, ST));
        dev::ew_reduce(c, (int)ell, mem, ell * nn, MODS, LOGN, ST);
        em = xm;  // keep alive
        dm = cm;
        launch = [&, c, x] {
            dev::modup_convert(x, c, (int)ell, (int)K, I.P.alpha, digits, mem, ell * nn, (size_t)digits * W * nn,
                               I.ext(ell), I.modup_tab, I.LT.modup_off[ell].data(), MODS, LOGN, ST, I.modup_fp,
                               I.LT.modup_fp_off[ell].data(), I.LT.modup_fp_mid);
        };
        bytes = (double)mem * (ell + (size_t)digits * W - ell) * B;
    } else if (name == "expand_uniform") {  // one digit's uniform half over all nq + K primes
        auto bm = I.alloc(I.P.nall() * nn * 8);
        u64 *a = static_cast<u64 *>(bm->p);
        em = bm;  // keep alive
        const PublicSeed seed{};
        launch = [&, a, seed] { expand_public(I, seed, 0, 0, a); };
        bytes = (double)I.P.nall() * B;  // written
    } else {
        throw std::invalid_argument("time_kernel: unknown kernel " + name);
    }
    launch();  // warm
    hipEvent_t e0, e1;
    HIP_OK(hipEventCreate(&e0));
    HIP_OK(hipEventCreate(&e1));
    HIP_OK(hipEventRecord(e0, ST));
    for (int i = 0; i < iters; ++i) launch();
    HIP_OK(hipEventRecord(e1, ST));
    HIP_OK(hipEventSynchronize(e1));
    float ms = 0;
    HIP_OK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    avg_ms = (double)ms / iters;
}

}  // namespace fhe
