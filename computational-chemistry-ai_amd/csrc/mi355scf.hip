// mi355scf.hip -- MI355X (gfx950 / CDNA4) SCF Fock-build engine: C ABI + HIP kernels.
//
// See include/mi355scf.h for the boundary and DESIGN.md for the data layout.  Kernels:
//   int1e_kernel            S, T, V, dipole (Obara-Saika overlap recurrences + Rys nuclear attraction)
//   eri_rys_kernel          contracted [e0|f0] integrals by Rys quadrature, one wave per shell quartet,
//                           2-D recurrence tables staged in LDS
//   eri_transform_scatter   HRR + cart->sph as two small dense products, scatter into 8^4 AO tiles
//   schwarz_diag_kernel     q_ab = sqrt(max (ab|ab))                      (row a3)
//   jk_tiles_kernel         one-pass J+K digestion of the HBM-resident tiles (rows a5, a6)
//   pad/finalize, DIIS helpers                                             (row a10)
//   pcm_* kernels           C-PCM surface-charge integrals, their two per-cycle passes and gradient (pcm.py)
// Written for gfx950 only: 64-lane waves are assumed throughout.

#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <string>
#include <thread>
#include <type_traits>
#include <mutex>
#include <map>
#include <unordered_map>
#include <vector>

#include "../../include/mi355scf.h"
#include "rys_tables.h"

#define LMAX 4      /* g shells: auxiliary (density-fitting) contexts only; orbital shells stop at f (LMAX_1E) */
#define LMAX_1E 3   /* one-electron / AO-value kernels: their per-thread blocks are sized for l <= f */
#define NPC ((LMAX + 1) * (LMAX + 2) / 2) /* pair classes (la>=lb) */
#define BLK 8
#define ATM_SLOTS 6
#define BAS_SLOTS 8

static thread_local std::string g_err;
static int fail(const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return -1;
}
#define HIPCHK(x)                                                                                   \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess) return fail("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

extern "C" const char *mi_last_error(void) { return g_err.c_str(); }

// -------------------------------------------------------------------------------------------------
// Device-memory pool for the MANY small and medium buffers of a context (pair records, matrices, directories, per-call
// scratch): a geometry step creates and destroys ~150 of them, and every hipMalloc / hipFree maps or unmaps pages and
// synchronises the device (38 ms for the mi_ctx_destroy of ibuprofen/def2-TZVP alone).  dev_free parks a block in a per-device
// free list by size class (device-synchronised first, like hipFree, so a parked block is never still being read), dev_malloc
// takes one from there.  Blocks above 1 GiB, the tile store (TileArena) and the hand-over buffers (Scratch) bypass the pool.
// At most POOL_CAP bytes are parked per device; mi_release_cache and an out-of-memory hipMalloc empty the pool.
// -------------------------------------------------------------------------------------------------
static const size_t POOL_CAP = (size_t)6 << 30, POOL_MAX_BLOCK = (size_t)1 << 30;
struct DevPool {
    std::mutex mu;
    std::unordered_map<void *, size_t> live;                  // pooled blocks handed out: pointer -> size class
    std::map<size_t, std::vector<void *>> parked;             // size class -> free blocks
    size_t parked_bytes = 0;
};
static DevPool g_pool[16];
static size_t pool_class(size_t n)
{
    if (n <= 256) return 256;
    size_t c = 256;
    while (c < n) c <<= 1;
    const size_t three_q = c / 4 * 3;                          // classes 2^k and 3 * 2^(k-2): at most 33 % of slack
    return (n <= three_q && three_q >= 256) ? three_q : c;
}
static void pool_flush(int dev)
{
    DevPool &P = g_pool[dev & 15];
    for (auto &kv : P.parked)
        for (void *q : kv.second) hipFree(q);
    P.parked.clear();
    P.parked_bytes = 0;
}
static hipError_t dev_malloc_impl(void **out, size_t n)
{
    int dev = 0;
    hipGetDevice(&dev);
    if (n > POOL_MAX_BLOCK) return hipMalloc(out, n);
    DevPool &P = g_pool[dev & 15];
    const size_t cls = pool_class(std::max<size_t>(n, 1));
    std::lock_guard<std::mutex> g(P.mu);
    auto it = P.parked.find(cls);
    if (it != P.parked.end() && !it->second.empty()) {
        *out = it->second.back();
        it->second.pop_back();
        P.parked_bytes -= cls;
        P.live[*out] = cls;
        return hipSuccess;
    }
    hipError_t e = hipMalloc(out, cls);
    if (e != hipSuccess) {                                    // out of memory: give the parked blocks back and try again
        (void)hipGetLastError();
        pool_flush(dev);
        e = hipMalloc(out, cls);
    }
    if (e == hipSuccess) P.live[*out] = cls;
    return e;
}
template <class T> static hipError_t dev_malloc(T **out, size_t n) { return dev_malloc_impl((void **)out, n); }
static hipError_t dev_free(void *q)
{
    if (!q) return hipSuccess;
    int dev = 0;
    hipGetDevice(&dev);
    DevPool &P = g_pool[dev & 15];
    size_t cls = 0;
    {
        std::lock_guard<std::mutex> g(P.mu);
        auto it = P.live.find(q);
        if (it != P.live.end()) { cls = it->second; P.live.erase(it); }
    }
    if (!cls) return hipFree(q);                               // not one of ours (large block, or allocated on another device)
    hipDeviceSynchronize();                                   // what hipFree would have done: nobody reads the block any more
    std::lock_guard<std::mutex> g(P.mu);
    if (P.parked_bytes + cls > POOL_CAP) return hipFree(q);
    P.parked[cls].push_back(q);
    P.parked_bytes += cls;
    return hipSuccess;
}
static size_t pool_parked_bytes(int dev) { DevPool &P = g_pool[dev & 15]; std::lock_guard<std::mutex> g(P.mu); return P.parked_bytes; }

// Host-side OpenMP is used only for the per-pair transformation matrices.  Idle workers must not spin
// (libomp's default 200 ms block time starves the Python/torch threads between calls).
static int g_rows_g32 = 1;   // (option grad_rows_g32) row gradient kernel: lane groups of 32 (two quartets per wave) up to 64 rows
static int host_threads()
{
    static int n = [] {
        setenv("KMP_BLOCKTIME", "0", 0);
        const char *e = getenv("MI355_HOST_THREADS");
        int v = e ? atoi(e) : 16;
        return v < 1 ? 1 : v;
    }();
    return n;
}
extern "C" int mi_abi_version(void) { return 2; }

// =================================================================================================
// Real solid harmonics (generic l): coefficients of the unit-normalised real harmonics r^l Y_lm in
// monomials x^a y^b z^c; order m=-l..l, except l=1 -> (x,y,z) (PySCF AO convention [MEM]).
// Formula: Helgaker, Jorgensen, Olsen, "Molecular Electronic-Structure Theory", eq. 6.4.47-6.4.50.
// =================================================================================================
static inline int ncart(int l) { return (l + 1) * (l + 2) / 2; }
static inline int cart_index(int l, int lx, int ly) /* order: lx desc, then ly desc */
{
    int n = 0;
    for (int x = l; x > lx; x--) n += l - x + 1;
    return n + (l - lx - ly);
}
static double fact(int n) { double f = 1; for (int i = 2; i <= n; i++) f *= i; return f; }
static double binom(int n, int k) { if (k < 0 || k > n) return 0; return fact(n) / (fact(k) * fact(n - k)); }

static void c2s_generic(int l, std::vector<double> &out) /* [ncart][2l+1] */
{
    int nc = ncart(l), ns = 2 * l + 1;
    out.assign((size_t)nc * ns, 0.0);
    for (int m = -l; m <= l; m++) {
        int am = std::abs(m);
        double N = 1.0 / (std::pow(2.0, am) * fact(l)) * std::sqrt(2.0 * fact(l + am) * fact(l - am) / (m == 0 ? 2.0 : 1.0));
        N *= std::sqrt((2 * l + 1) / (4.0 * M_PI));
        int col = (l == 1) ? (m == 1 ? 0 : (m == -1 ? 1 : 2)) : (m + l);
        for (int t = 0; t <= (l - am) / 2; t++)
            for (int u = 0; u <= t; u++) {
                /* v = vm, vm+1, ... with 2v <= am ; vm = 0 (m>=0) or 1/2 (m<0): use v2 = 2v */
                for (int v2 = (m < 0 ? 1 : 0); v2 <= am; v2 += 2) {
                    double C = std::pow(-1.0, t + (v2 - (m < 0 ? 1 : 0)) / 2) * std::pow(0.25, t) * binom(l, t) *
                               binom(l - t, am + t) * binom(t, u) * binom(am, v2);
                    int px = 2 * t + am - 2 * u - v2, py = 2 * u + v2, pz = l - 2 * t - am;
                    if (px < 0 || py < 0 || pz < 0) continue;
                    out[(size_t)cart_index(l, px, py) * ns + col] += N * C;
                }
            }
    }
}

extern "C" int mi_c2s_table(int l, double *out)
{
    if (l < 0 || l > 6) return fail("mi_c2s_table: l=%d out of range", l);
    std::vector<double> c;
    c2s_generic(l, c);
    memcpy(out, c.data(), c.size() * sizeof(double));
    return 0;
}

// =================================================================================================
// Rys roots and weights from the generated Chebyshev tables (host + device versions)
// =================================================================================================
struct RysDev {
    const double *cheb;   // RYS_CHEB
    const double *herm_r; // [(NMAX+1)*NMAX]
    const double *herm_w;
    int off[RYS_NMAX + 2];
    int nint[RYS_NMAX + 1];
};

// Chebyshev series of degree RYS_DEG at s in [-1, 1] (Clenshaw): every evaluation of a root / weight function, host and device
__host__ __device__ inline double rys_clenshaw(const double *c, double s)
{
    double b1 = 0.0, b2 = 0.0;
    const double s2 = 2.0 * s;
#pragma unroll
    for (int k = RYS_DEG; k >= 1; k--) {
        const double t = s2 * b1 - b2 + c[k];
        b2 = b1;
        b1 = t;
    }
    return s * b1 - b2 + c[0];
}
// interval of x in a table of `nint` intervals of width RYS_H, and the series argument inside it
__host__ __device__ inline int rys_interval(double x, int nint, double &s)
{
    int iv = (int)(x * (1.0 / RYS_H));
    if (iv >= nint) iv = nint - 1;
    s = (x - (iv * RYS_H + 0.5 * RYS_H)) * (2.0 / RYS_H);
    return iv;
}

template <class T>
__device__ inline double rys_eval_impl(const T &R, int n, int f, double x)
{
    int ni = R.nint[n];
    if (x < ni * RYS_H) {
        double s;
        const int iv = rys_interval(x, ni, s);
        return rys_clenshaw(R.cheb + R.off[n] + (size_t)(iv * 2 * n + f) * (RYS_DEG + 1), s);
    }
    if (f < n) return R.herm_r[n * RYS_NMAX + f] / x;
    return R.herm_w[n * RYS_NMAX + (f - n)] * rsqrt(x);
}
__device__ inline double rys_eval(const RysDev &R, int n, int f, double x) { return rys_eval_impl(R, n, f, x); }

extern "C" int mi_rys_roots_host(int n, double x, double *roots, double *weights)
{
    if (n < 1 || n > RYS_NMAX) return fail("nroots out of range");
    struct H { const double *cheb, *herm_r, *herm_w; int off[RYS_NMAX + 2]; int nint[RYS_NMAX + 1]; } R;
    R.cheb = RYS_CHEB_H; R.herm_r = &RYS_HERM_R_H[0][0]; R.herm_w = &RYS_HERM_W_H[0][0];
    for (int i = 0; i <= RYS_NMAX; i++) { R.off[i] = i == 0 ? 0 : RYS_OFFSET_H[i]; R.nint[i] = RYS_NINT_H[i]; }
    for (int f = 0; f < n; f++) {
        // host path: rys_eval_impl's branches with std:: functions
        int ni = R.nint[n];
        for (int pass = 0; pass < 2; pass++) {
            int ff = f + pass * n;
            double val;
            if (x < ni * RYS_H) {
                double s;
                const int iv = rys_interval(x, ni, s);
                val = rys_clenshaw(R.cheb + R.off[n] + (size_t)(iv * 2 * n + ff) * (RYS_DEG + 1), s);
            } else if (pass == 0) val = R.herm_r[n * RYS_NMAX + f] / x;
            else val = R.herm_w[n * RYS_NMAX + f] / std::sqrt(x);
            (pass == 0 ? roots : weights)[f] = val;
        }
    }
    return 0;
}

// =================================================================================================
// Context
// =================================================================================================
struct ShellH {
    int atom, l, nprim, ao;   // ao: first AO in the TILE order of the ERI store (see set_tile_order); ao_nat: in the caller's order
    int ao_nat;
    const double *exps, *coef;
    double r[3];
};

struct PairRec { // one shell pair (l_i >= l_j)
    int sh_i, sh_j, ao_i, ao_j;
    int prim_off, nprim; // primitive pairs: 8 doubles each {p,Px,Py,Pz,PAx,PAy,PAz,K}
    int m_off;           // offset (doubles) of the [ns_i*ns_j][ne] HRR*c2s matrix
    int pad;
};

struct PairClass {
    // gradient variants of each (sorted) pair: [orientation 0: first = sh_i | 1: first = sh_j][0: l+1 | 1: l-1]
    std::vector<PairRec> g_recs[2][2];
    PairRec *d_g_recs[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    int la, lb;
    int ne;                        // number of [e0| cartesian components, e = la..la+lb
    int nsab;                      // (2la+1)(2lb+1)
    std::vector<PairRec> recs;     // sorted by q desc after Schwarz
    std::vector<double> q;         // Schwarz bound per rec
    std::vector<double> cq;        // non-increasing along the sorted list: max q over the rec's cluster (== q without clustering)
    PairRec *d_recs = nullptr;
    double *d_q = nullptr;
    // primitive-pair counts of the sorted list: mean, and mean over windows of 4 consecutive pairs of the window maximum
    // (four consecutive tasks share a wave in the 16-lane-group kernels and run as long as the longest of them)
    double mean_np = 1.0, max4_np = 1.0;
    int max_np = 1;                // largest primitive-pair count of a pair of the class
};

struct TileInfo { int I, J, K, L; };
struct RunRec { int J, K, L, first, count; };

// ---- tile geometry.  A tile (I J|K L) is a list of rows (j, m) -- j = 0..7, m = l-pair 0..3, j-major -- of 16-byte chunks
// {T[i,j,k,2m], T[i,j,k,2m+1]}, the chunks of a row ordered (i, k).  Off the block diagonals a row holds all bi*bk lanes.
// Where I == J only i >= j is stored (weight 1 off the diagonal, 1/2 on it: the kernels' contractions are symmetric in
// (i,j) for a symmetric density, so the dropped half would only repeat the kept one), where K == L only k >= 2m (elements
// with k < l inside a kept chunk are zero).  Rows shrink accordingly and stay contiguous in lane order, so every load of the
// digestion kernel is still a coalesced run of 16-byte chunks; the two-fold redundancy of diagonal tiles is gone from the stream.
__host__ __device__ inline int tile_i0(bool dij, int j, int bi) { return dij ? (j < bi ? j : bi) : 0; }
__host__ __device__ inline int tile_k0(bool dkl, int m, int bk) { return dkl ? (2 * m < bk ? 2 * m : bk) : 0; }
__host__ __device__ inline int tile_pi(bool dij, int j, int bi)   // rows of i-lanes before row j
{
    if (!dij) return j * bi;
    const int jc = j < bi ? j : bi;
    return jc * bi - jc * (jc - 1) / 2;
}
__host__ __device__ inline int tile_qk(bool dkl, int m, int bk)   // k-lanes per i in the l-pairs before m
{
    if (!dkl) return m * bk;
    int q = 0;
    for (int mm = 0; mm < m; mm++) q += bk - tile_k0(true, mm, bk);
    return q;
}
__host__ __device__ inline int tile_chunks(bool dij, bool dkl, int bi, int bk) { return tile_pi(dij, BLK, bi) * tile_qk(dkl, 4, bk); }
// chunk index of (ii, jj, kk, m) inside its tile, -1 when that lane is not stored
__host__ __device__ inline int tile_chunk(bool dij, bool dkl, int bi, int bk, int ii, int jj, int kk, int m)
{
    const int i0 = tile_i0(dij, jj, bi), k0 = tile_k0(dkl, m, bk);
    if (ii < i0 || kk < k0) return -1;
    return tile_pi(dij, jj, bi) * tile_qk(dkl, 4, bk) + (bi - i0) * tile_qk(dkl, m, bk) + (ii - i0) * (bk - k0) + (kk - k0);
}
// offset in doubles of element (ii,jj,kk,ll) and the weight it is stored with (0: not stored)
// tri = false: the round-1 layout (full rows everywhere, 1/2 per block coincidence on both mirror elements)
__host__ __device__ inline int64_t tile_elem(bool tri, bool dij, bool dkl, bool dpp, int bi, int bk, int ii, int jj, int kk, int ll, double *w)
{
    double wt = dpp ? 0.5 : 1.0;
    if (!tri) {
        if (dij) wt *= 0.5;
        if (dkl) wt *= 0.5;
        *w = wt;
        return (int64_t)tile_chunk(false, false, bi, bk, ii, jj, kk, ll >> 1) * 2 + (ll & 1);
    }
    if (dij) { if (ii < jj) { *w = 0.0; return -1; } if (ii == jj) wt *= 0.5; }
    if (dkl) { if (kk < ll) { *w = 0.0; return -1; } if (kk == ll) wt *= 0.5; }
    *w = wt;
    return (int64_t)tile_chunk(dij, dkl, bi, bk, ii, jj, kk, ll >> 1) * 2 + (ll & 1);
}

struct mi_ctx {
    int device = 0;
    int natm = 0, nbas = 0, nao = 0, nblk = 0, npad = 0;
    std::vector<int32_t> atm, bas;
    std::vector<double> env;
    std::vector<ShellH> shells;
    // device-side basis for 1e kernel
    double *d_env = nullptr;
    int32_t *d_bas = nullptr, *d_atm = nullptr;
    int *d_shell_ao = nullptr;
    double *d_shell_xyz = nullptr;       // [nbas][3]
    double *d_c2s = nullptr;             // concatenated c2s tables l=0..LMAX
    int c2s_off[LMAX + 2];
    RysDev rys;                          // device pointers inside
    double *d_rys_cheb = nullptr, *d_herm_r = nullptr, *d_herm_w = nullptr;
    // shell pairs grouped by angular class for the one-electron and PCM launches (shell_pair_classes): [0] i >= j with the
    // higher l first, [1] all ordered (i, j); class k = la * 4 + lb is rows start[k] .. start[k + 1] of pairs [n][2]
    struct PairClasses { std::vector<int> pairs; int start[17] = {}; int *d_pairs = nullptr; } pair_classes[2];
    // pairs
    PairClass pc[NPC];
    double *d_prim = nullptr;            // all primitive-pair records
    double *d_M = nullptr;               // all transformation matrices
    std::vector<double> h_prim, h_M;     // host copies (gradient variants are appended lazily)
    double tol = 1e-13;
    int rank = 0, nranks = 1;
    bool grad_ready = false;
    // host half of prepare_grad_records (variant records, derivative matrices: 0.08-0.1 s for ibuprofen/def2-TZVP) on a helper
    // thread started at the end of mi_eri_prepare (`grad_prefetch`): it overlaps the SCF loop of a geometry step
    std::thread grad_worker;
    bool grad_host_ready = false;
    int grad_host_rc = 0;
    std::string grad_host_err;
    int opt_grad_prefetch = 0;
    // component index tables per class quadruple (built lazily)
    // tiles
    int64_t n_tiles = 0;
    std::vector<TileInfo> tiles;
    std::vector<int64_t> tile_off;
    std::vector<RunRec> runs;
    int32_t *d_tile_table = nullptr;     // [nbp(nbp+1)/2] -> local tile index or -1
    uint8_t *d_tile_present = nullptr;   // sharded contexts only: 1 where the slot is resident on another rank
    int64_t *d_tile_off = nullptr;
    int *d_tile_I = nullptr;
    RunRec *d_runs = nullptr;
    RunRec *d_segs = nullptr;            // runs cut at wave boundaries
    int *d_wave_seg = nullptr;           // [nwaves+1] segment range of each wave
    int n_jk_waves = 0;
    int n_jk_segs = 0;                   // J/K work items (entries of d_segs)
    int n_jk_cached = 0;                 // leading J/K work items kept in the Infinity Cache (default-policy loads)
    double *d_tiles = nullptr;
    int64_t tile_doubles = 0, tile_alloc = 0;
    // J/K work buffers
    double *d_Dpad = nullptr, *d_Jacc = nullptr, *d_Kacc = nullptr;
    int ldp = 0;
    // mi_build_jk_multi: padded densities and accumulators of one batch (JKM_BATCH of each), allocated on first use
    double *d_mDpad = nullptr, *d_mJacc = nullptr, *d_mKacc = nullptr;
    double *d_red = nullptr;
    mi_eri_stats stats{};
    int64_t mem_need_bytes = 0, mem_free_bytes = 0; // of the last mi_eri_prepare (also when it returned MI_ERR_NOMEM)
    bool eri_ready = false;
    // tunables (mi_set_option)
    int opt_runmax = 0;      // tiles per J/K work item (0 = auto: ntiles/2048 clamped to [8,64])
    double opt_omega = 0.0;  // > 0: the next mi_eri_prepare stores erf(omega r12)/r12 integrals (long-range store)
    double eri_omega = 0.0;  // omega of the current store (0: full Coulomb)
    int opt_jk_waves = 0;    // 0: one wave per work item, longest first; >0: that many waves, equal-cost shares
    int opt_jk_nt = 1;       // nontemporal loads for the tile stream
    double opt_grad_dtol = 1e-13; // gradient: skip quartets with q_ab q_cd max|G| below this (0: Schwarz only)
    int opt_xf_mfma_min = 300; // transform kernel: MFMA tiles only when the spherical block has at least this many elements
    double opt_tpq_maxprim = 32.0; // thread-per-quartet kernels only when the mean primitive quartets per shell quartet stay below this
    int64_t opt_tpq_min_tasks = 32768; // ... and the class pair has at least this many quartets (a smaller launch leaves the device idle)
    int opt_eri_tpq = 1;     // thread-per-quartet fused ERI kernels for the low angular classes (0: wave-per-quartet pair everywhere)
    int opt_jk_multi_batch = 8;  // mi_build_jk_multi: densities per launch (1..JKM_BATCH); 8 measured faster per density than 16
    int opt_jk_pair = -1;    // n_dm = 2: one pass with two waves per work item (-1: for stores > 16 GB, 0: one pass per density, 1: always)
    int opt_tri_tiles = 1;   // block-diagonal tiles store triangular rows (0: the full-row layout of round 1); next mi_eri_prepare
    int tri = 1;             // layout of the current store
    int opt_jk_cache_mb = 160; // MiB of tiles read with the default cache policy when the tensor exceeds the Infinity Cache (0: none)
    int opt_grad_rows = 1;   // gradient: row kernel (eri_grad_rows_kernel) for the classes it covers
    int opt_grad_rows_min = 20;  // ... when the two derivative blocks have at least this many rows
    int opt_grad_live = 1;   // gradient: wave-per-quartet launches walk the compacted list of density-screened quartets
    int opt_jk_kjlt = 0;     // J+K: K_JL reduced per tile instead of run-wide accumulators (two waves per SIMD), experiment
    int opt_jk_dpp = 1;      // per-tile reduce-scatters of the J/K kernel through DPP moves (0: ds_bpermute, the round-1/2 path)
    int opt_jk_pipe = -1;    // software-pipelined half-tile kernel for the K-carrying builds (-1: when the tensor is cache-resident)
    int opt_ao_order = 1;    // tile AO order: 1 = angular-momentum major (all s, all p, ... ; tiles become class-homogeneous), 0 = caller's
    int opt_ket_cluster = 1; // kets ordered by (block pair of the store, shell) inside Schwarz-ordered clusters instead of by q alone
    int opt_xf_mlds = 0;     // transform kernel: stage the per-pair matrices in LDS when a quartet's blocks then fit this many KB (0: never; measured 1.3-3x SLOWER at 16-96)
    int opt_rys_qpw_maxcomp = 256;   // Rys kernel: four quartets per wave for classes up to this many [e0|f0] components ...
    double opt_rys_qpw_maxprim = 4.0; // ... whose quartets have at most about this many primitive quartets (0 components: off)
    int opt_xf_qpw_max = 40;         // transform kernel: four quartets per wave up to this many spherical elements per quartet
    // MiB of the [e0|f0] hand-over buffer between the Rys and the transform launches, and of each of the two buffers of the
    // gradient.  Measured on ibuprofen/def2-TZVP (tools/eri_bench.py, ERI_OPTS): 12 / 48 / 256 / 1024 / 4096 MiB -> evaluation
    // 0.53 / 0.38 / 0.353 / 0.353 / 0.339 s, gradient (2 x half of that) 3.9 / 2.1 / 1.23 / 1.14 / 1.11 s: few large launches beat
    // many small ones (drain + ramp of latency-bound waves per launch); keeping a batch inside the Infinity Cache buys nothing
    int opt_work_mb = 2048;
    int opt_grad_work_mb = 1024;
    int opt_vmat_fold_mt = 3;   // xc_vmat_fold: 64-row tiles per workgroup (1..5)
    int opt_rys_fine = 1;    // Rys kernel: also 2 and 8 components per lane (fewer registers, more waves for the classes in between)
    int opt_eri_fused = 0;   // mid / high classes: fused Rys + transform + scatter kernel (1) instead of the two-launch pair with its hand-over buffer -- measured SLOWER (0.273 vs 0.245 s): default off
    int opt_task_table = 1;  // wave-per-quartet kernels read (bra, ket) of a task from a table written once per class pair
    int opt_prim_lds = 0;    // Rys kernel: primitive-pair records of the quartet staged in LDS
    int opt_xcd_map = 1;     // ERI kernels: consecutive task chunks stay on one XCD (its L2 merges the pieces of a line)
    int opt_df_batch_max = 0; // mi_df_build / mi_df_grad: at most this many tasks per pass of a class (0: only the hand-over buffer limits a pass)
    int ao_order = 0;       // order of the current shells[].ao / d_perm
    int *d_perm = nullptr, *d_iperm = nullptr;   // caller AO -> tile AO and back
    std::vector<int> perm, iperm;
    int opt_vmat_xcd = 1;    // xc_vmat: XCD-aware workgroup order (tiles of one split share an XCD's L2)
    int opt_vmat_wgs = 0;    // xc_vmat: workgroups aimed at by the split over the grid points (0: 1024 = two per CU; -1: round-1 formula)
    int opt_sp2_direct = 0;  // planned purification, one launch per pass: 1 = sp2_direct_kernel (MFMA operands loaded straight into
                             // registers, N <= 320), 0 = sp2_plan_kernel (row panels staged in LDS)
    double *d_xt_scratch = nullptr; // xc_tail_kernel: per-workgroup partials + ticket
};

static inline int pc_index(int la, int lb) { return la * (la + 1) / 2 + lb; }
static inline int ne_of(int la, int lb) { int n = 0; for (int e = la; e <= la + lb; e++) n += ncart(e); return n; }

static double gaussian_int(int n, double a) { return std::tgamma((n + 1) * 0.5) / (2.0 * std::pow(a, (n + 1) * 0.5)); }

// AO order of the ERI store ("tile order").  order 0: the caller's (shell by shell as in `bas`).  order 1: angular-momentum
// major -- all s shells, then all p, d, f (shells of one l in the caller's sequence) -- so that an 8-AO block holds shells of
// ONE l (but for three boundary blocks): every tile then belongs to one angular class, and the pieces of a 64-byte line of the
// store (4 consecutive k x one l pair) come from quartets of the SAME class, i.e. of one launch, which lets neighbouring
// lanes / workgroups complete the line together.  The permutation is internal: densities are gathered into
// tile order when they are padded, J / K / F are scattered back by the finalize kernels.
static int set_tile_order(mi_ctx *c, int order)
{
    if (c->ao_order == order) return 0;
    const int nbas = c->nbas;
    std::vector<int> seq(nbas);
    std::iota(seq.begin(), seq.end(), 0);
    if (order == 1) std::stable_sort(seq.begin(), seq.end(), [&](int a, int b) { return c->shells[a].l < c->shells[b].l; });
    c->perm.assign(std::max(c->nao, 1), 0);
    c->iperm.assign(std::max(c->nao, 1), 0);
    int pos = 0;
    for (int s_ : seq) {
        ShellH &S = c->shells[s_];
        S.ao = pos;
        for (int m = 0; m < 2 * S.l + 1; m++) { c->perm[S.ao_nat + m] = pos + m; c->iperm[pos + m] = S.ao_nat + m; }
        pos += 2 * S.l + 1;
    }
    HIPCHK(hipMemcpy(c->d_perm, c->perm.data(), sizeof(int) * c->perm.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->d_iperm, c->iperm.data(), sizeof(int) * c->iperm.size(), hipMemcpyHostToDevice));
    c->ao_order = order;
    return 0;
}

struct HostStash {
    std::mutex mu;
    std::vector<double> h_M, h_prim;
    std::vector<TileInfo> tiles;
    std::vector<int64_t> tile_off;
};
static HostStash g_stash[16];

// Shell pairs grouped by angular class, built and uploaded once per context: ordered = 0: i >= j, stored with the higher l
// first (S/T/V/dipole, B), 1: all (i, j) (gradients, derivative on i).  A context with shells beyond f (auxiliary basis) keeps
// empty lists: every reader refuses it first (check_orbital_lmax).
static int shell_pair_classes(mi_ctx *c, int ordered)
{
    mi_ctx::PairClasses &pc = c->pair_classes[ordered];
    std::vector<std::vector<int>> by(16);
    bool orbital = true;
    for (const ShellH &s : c->shells) orbital = orbital && s.l <= LMAX_1E;
    for (int i = 0; orbital && i < c->nbas; i++)
        for (int j = 0; j < (ordered ? c->nbas : i + 1); j++) {
            int a = i, b = j;
            if (!ordered && c->shells[a].l < c->shells[b].l) std::swap(a, b);
            by[c->shells[a].l * 4 + c->shells[b].l].push_back(a);
            by[c->shells[a].l * 4 + c->shells[b].l].push_back(b);
        }
    for (int k = 0; k < 16; k++) {
        pc.start[k] = (int)pc.pairs.size() / 2;
        pc.pairs.insert(pc.pairs.end(), by[k].begin(), by[k].end());
    }
    pc.start[16] = (int)pc.pairs.size() / 2;
    HIPCHK(dev_malloc(&pc.d_pairs, sizeof(int) * std::max<size_t>(pc.pairs.size(), 2)));
    HIPCHK(hipMemcpy(pc.d_pairs, pc.pairs.data(), sizeof(int) * pc.pairs.size(), hipMemcpyHostToDevice));
    return 0;
}

extern "C" int mi_ctx_create(const int32_t *atm, int natm, const int32_t *bas, int nbas, const double *env,
                             int nenv, int device_id, mi_ctx **out)
{
    if (!atm || !bas || !env || !out || natm <= 0 || nbas <= 0) return fail("mi_ctx_create: bad arguments");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail("mi_ctx_create: no HIP device available (this engine has no CPU fallback)");
    if (device_id < 0 || device_id >= ndev) return fail("mi_ctx_create: device %d out of range (have %d)", device_id, ndev);
    HIPCHK(hipSetDevice(device_id));
    mi_ctx *c = new mi_ctx();
    c->device = device_id;
    c->natm = natm; c->nbas = nbas;
    c->atm.assign(atm, atm + (size_t)natm * ATM_SLOTS);
    c->bas.assign(bas, bas + (size_t)nbas * BAS_SLOTS);
    c->env.assign(env, env + nenv);
    int ao = 0;
    std::vector<int> shell_ao(nbas + 1);
    for (int i = 0; i < nbas; i++) {
        const int32_t *b = bas + (size_t)i * BAS_SLOTS;
        if (b[3] != 1) { delete c; return fail("shell %d: nctr=%d unsupported (split general contractions)", i, b[3]); }
        if (b[1] < 0 || b[1] > LMAX) { delete c; return fail("shell %d: l=%d unsupported (max %d)", i, b[1], LMAX); }
        ShellH s;
        s.atom = b[0]; s.l = b[1]; s.nprim = b[2]; s.ao = ao; s.ao_nat = ao;
        s.exps = c->env.data() + b[5]; s.coef = c->env.data() + b[6];
        const double *r = c->env.data() + atm[(size_t)s.atom * ATM_SLOTS + 1];
        s.r[0] = r[0]; s.r[1] = r[1]; s.r[2] = r[2];
        c->shells.push_back(s);
        shell_ao[i] = ao;
        ao += 2 * s.l + 1;
    }
    shell_ao[nbas] = ao;
    c->nao = ao;
    c->nblk = (ao + BLK - 1) / BLK;
    c->npad = c->nblk * BLK;
    c->ldp = c->npad + BLK;
    // device copies
    HIPCHK(dev_malloc(&c->d_env, sizeof(double) * nenv));
    HIPCHK(hipMemcpy(c->d_env, env, sizeof(double) * nenv, hipMemcpyHostToDevice));
    HIPCHK(dev_malloc(&c->d_bas, sizeof(int32_t) * nbas * BAS_SLOTS));
    HIPCHK(hipMemcpy(c->d_bas, bas, sizeof(int32_t) * nbas * BAS_SLOTS, hipMemcpyHostToDevice));
    HIPCHK(dev_malloc(&c->d_atm, sizeof(int32_t) * natm * ATM_SLOTS));
    HIPCHK(hipMemcpy(c->d_atm, atm, sizeof(int32_t) * natm * ATM_SLOTS, hipMemcpyHostToDevice));
    HIPCHK(dev_malloc(&c->d_shell_ao, sizeof(int) * (nbas + 1)));
    HIPCHK(hipMemcpy(c->d_shell_ao, shell_ao.data(), sizeof(int) * (nbas + 1), hipMemcpyHostToDevice));
    {
        std::vector<double> xyz((size_t)nbas * 3);
        for (int i = 0; i < nbas; i++)
            for (int d = 0; d < 3; d++) xyz[3 * i + d] = c->shells[i].r[d];
        HIPCHK(dev_malloc(&c->d_shell_xyz, sizeof(double) * xyz.size()));
        HIPCHK(hipMemcpy(c->d_shell_xyz, xyz.data(), sizeof(double) * xyz.size(), hipMemcpyHostToDevice));
    }
    // c2s tables
    std::vector<double> all;
    for (int l = 0; l <= LMAX; l++) {
        std::vector<double> t;
        c2s_generic(l, t);
        c->c2s_off[l] = (int)all.size();
        all.insert(all.end(), t.begin(), t.end());
    }
    c->c2s_off[LMAX + 1] = (int)all.size();
    HIPCHK(dev_malloc(&c->d_c2s, sizeof(double) * all.size()));
    HIPCHK(hipMemcpy(c->d_c2s, all.data(), sizeof(double) * all.size(), hipMemcpyHostToDevice));
    if (shell_pair_classes(c, 0) || shell_pair_classes(c, 1)) return -1;
    // Rys tables
    HIPCHK(dev_malloc(&c->d_rys_cheb, sizeof(double) * RYS_CHEB_SIZE));
    HIPCHK(hipMemcpy(c->d_rys_cheb, RYS_CHEB_H, sizeof(double) * RYS_CHEB_SIZE, hipMemcpyHostToDevice));
    HIPCHK(dev_malloc(&c->d_herm_r, sizeof(RYS_HERM_R_H)));
    HIPCHK(hipMemcpy(c->d_herm_r, RYS_HERM_R_H, sizeof(RYS_HERM_R_H), hipMemcpyHostToDevice));
    HIPCHK(dev_malloc(&c->d_herm_w, sizeof(RYS_HERM_W_H)));
    HIPCHK(hipMemcpy(c->d_herm_w, RYS_HERM_W_H, sizeof(RYS_HERM_W_H), hipMemcpyHostToDevice));
    c->rys.cheb = c->d_rys_cheb; c->rys.herm_r = c->d_herm_r; c->rys.herm_w = c->d_herm_w;
    for (int i = 0; i <= RYS_NMAX + 1; i++) c->rys.off[i] = RYS_OFFSET_H[i];
    for (int i = 0; i <= RYS_NMAX; i++) c->rys.nint[i] = RYS_NINT_H[i];
    // shift: RYS_OFFSET_H[n] is the offset of block n (n>=1) -- see generator: offs[0]=0 is block 1.
    for (int n = 1; n <= RYS_NMAX; n++) c->rys.off[n] = RYS_OFFSET_H[n];
    // J/K buffers
    size_t pp = (size_t)c->ldp * c->ldp;
    // two of each: the spin pair of UHF / UKS is digested by one launch (jk_tiles_pair_kernel)
    HIPCHK(dev_malloc(&c->d_Dpad, sizeof(double) * 2 * pp));
    HIPCHK(dev_malloc(&c->d_Jacc, sizeof(double) * 2 * pp));
    HIPCHK(dev_malloc(&c->d_Kacc, sizeof(double) * 2 * pp));
    HIPCHK(dev_malloc(&c->d_red, sizeof(double) * 4096));
    HIPCHK(dev_malloc(&c->d_perm, sizeof(int) * std::max(ao, 1)));
    HIPCHK(dev_malloc(&c->d_iperm, sizeof(int) * std::max(ao, 1)));
    c->ao_order = -1;
    if (set_tile_order(c, 0)) { return -1; }
    {   // large host vectors left behind by the previous context of this device (mi_ctx_destroy): capacity without page faults
        HostStash &H = g_stash[c->device & 15];
        std::lock_guard<std::mutex> g(H.mu);
        H.h_M.clear(); H.h_prim.clear(); H.tiles.clear(); H.tile_off.clear();
        c->h_M.swap(H.h_M); c->h_prim.swap(H.h_prim); c->tiles.swap(H.tiles); c->tile_off.swap(H.tile_off);
    }
    *out = c;
    return 0;
}

// The resident tile store can be ~100 GB; hipMalloc of that size costs 0.1-2 s.  A freed store is parked
// (one slot per device) and reused by the next context -- e.g. every step of a geometry optimisation.
struct TileArena { double *ptr = nullptr; int64_t doubles = 0; };
static TileArena g_arena[16];
static std::vector<int64_t> g_arena_alloc_bytes;   // size of every fresh tile-store allocation of this process

static int arena_take(int dev, int64_t need, double **out)
{
    TileArena &a = g_arena[dev & 15];
    if (a.ptr && a.doubles >= need && a.doubles <= need + need / 4 + (1 << 20)) {
        *out = a.ptr; a.ptr = nullptr; a.doubles = 0;
        return 0;
    }
    if (a.ptr) { hipFree(a.ptr); a.ptr = nullptr; a.doubles = 0; }
    if (hipMalloc((void **)out, sizeof(double) * need) != hipSuccess) {   // the pool's parked blocks may be what is missing
        (void)hipGetLastError();
        { std::lock_guard<std::mutex> g(g_pool[dev & 15].mu); pool_flush(dev); }
        HIPCHK(hipMalloc((void **)out, sizeof(double) * need));
    }
    g_arena_alloc_bytes.push_back((int64_t)sizeof(double) * need);
    return 0;
}
// Fresh device allocations of tile stores of at least `min_bytes` made by this process (a parked store that is reused does
// not count): a geometry optimisation should show ONE large one for all its steps (the atomic-guess engines make tiny ones).
extern "C" int64_t mi_tile_store_allocations(int64_t min_bytes)
{
    int64_t n = 0;
    for (int64_t b : g_arena_alloc_bytes) n += b >= min_bytes;
    return n;
}

static void arena_give(int dev, double *p, int64_t doubles)
{
    TileArena &a = g_arena[dev & 15];
    if (a.ptr) hipFree(a.ptr);
    a.ptr = p; a.doubles = doubles;
}

// Scratch buffers that every mi_eri_prepare / mi_grad_eri of a geometry optimisation would otherwise allocate and free again
// (2 GB hand-over buffer, 2 x 1 GB for the gradient, task lists of a few hundred MB): kept per device between calls.  One slot
// per purpose; a slot that is in use (a second context working on the same device from another thread) is not shared -- the
// caller then gets a private allocation that is freed on return.  hipMalloc / hipFree of these sizes cost 30-150 ms per
// geometry step on the slower boxes of the pool.
enum { SCR_EVAL_WORK = 0, SCR_EVAL_TASKS, SCR_GRAD_WP, SCR_GRAD_WM, SCR_GRAD_TASKS, SCR_GRAD_LIVE, SCR_NSLOT };
struct ScratchSlot { void *p = nullptr; size_t bytes = 0; bool busy = false; };
static ScratchSlot g_scratch[16][SCR_NSLOT];
static std::mutex g_scratch_mu;
struct Scratch {   // RAII handle of one slot (or of a private allocation)
    int dev = 0, slot = -1;
    void *p = nullptr;
    size_t bytes = 0;
    bool cached = false;
    ~Scratch() { release(); }
    // at least `need` bytes, contents undefined; grows by 25 % when it has to (a grown cached slot stays grown)
    int ensure(int dev_, int slot_, size_t need)
    {
        if (p && bytes >= need) return 0;
        if (slot < 0) {
            dev = dev_; slot = slot_;
            std::lock_guard<std::mutex> g(g_scratch_mu);
            ScratchSlot &S = g_scratch[dev & 15][slot];
            if (!S.busy) { S.busy = true; cached = true; p = S.p; bytes = S.bytes; }
        }
        if (p && bytes >= need) return 0;
        if (p) { hipFree(p); p = nullptr; bytes = 0; }
        if (cached) { std::lock_guard<std::mutex> g(g_scratch_mu); g_scratch[dev & 15][slot].p = nullptr; g_scratch[dev & 15][slot].bytes = 0; }
        const size_t want = need + need / 4;
        if (hipMalloc(&p, want) != hipSuccess) { p = nullptr; return fail("out of device memory for a %zu-byte scratch buffer", want); }
        bytes = want;
        if (cached) { std::lock_guard<std::mutex> g(g_scratch_mu); g_scratch[dev & 15][slot].p = p; g_scratch[dev & 15][slot].bytes = bytes; }
        return 0;
    }
    void release()
    {
        if (slot < 0) return;
        if (cached) { std::lock_guard<std::mutex> g(g_scratch_mu); g_scratch[dev & 15][slot].busy = false; }
        else if (p) hipFree(p);
        p = nullptr; bytes = 0; slot = -1; cached = false;
    }
};

template <class T>
static int upload(T **dst, const std::vector<T> &v)
{
    if (*dst) { dev_free(*dst); *dst = nullptr; }
    size_t n = std::max<size_t>(v.size(), 1);
    HIPCHK(dev_malloc_impl((void **)dst, sizeof(T) * n));
    if (!v.empty()) HIPCHK(hipMemcpy(*dst, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
    return 0;
}

// Owning handle of a function-local device buffer (a block of the pool): given back when the call ends, whichever way.
// Buffers owned by a context (mi_ctx::d_*) are not DevBufs; they live until free_eri / mi_ctx_destroy.  dev_free synchronises
// the device, so a DevBuf that a loop reuses is declared outside the loop and grown with reserve().
template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;   // elements
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { reset(); }
    void reset() { if (p) dev_free(p); p = nullptr; cap = 0; }
    T *get() const { return p; }
    operator T *() const { return p; }
    hipError_t alloc(size_t n)   // contents undefined
    {
        reset();
        const hipError_t e = dev_malloc(&p, sizeof(T) * n);
        if (e == hipSuccess) cap = n; else p = nullptr;
        return e;
    }
    // room for n elements, contents undefined; a buffer that has to grow doubles (task prefixes of class pair after class pair)
    hipError_t reserve(size_t n) { return n > cap ? alloc(2 * n) : hipSuccess; }
    int upload(const std::vector<T> &v)
    {
        cap = 0;
        if (::upload(&p, v)) return -1;
        cap = std::max<size_t>(v.size(), 1);
        return 0;
    }
};

extern "C" void mi_release_cache(void)
{
    {
        std::lock_guard<std::mutex> g(g_scratch_mu);
        for (auto &dv : g_scratch)
            for (auto &S : dv)
                if (!S.busy && S.p) { hipFree(S.p); S.p = nullptr; S.bytes = 0; }
    }
    for (auto &a : g_arena) { if (a.ptr) hipFree(a.ptr); a.ptr = nullptr; a.doubles = 0; }
    for (int d = 0; d < 16; d++) { std::lock_guard<std::mutex> g(g_pool[d].mu); if (g_pool[d].parked_bytes) { hipSetDevice(d); pool_flush(d); } }
}

static void free_eri(mi_ctx *c)
{
    if (c->grad_worker.joinable()) c->grad_worker.join();
    c->grad_host_ready = false;
    if (c->d_tiles) { arena_give(c->device, c->d_tiles, c->tile_alloc); c->d_tiles = nullptr; }
    for (int i = 0; i < NPC; i++) {
        if (c->pc[i].d_recs) dev_free(c->pc[i].d_recs);
        if (c->pc[i].d_q) dev_free(c->pc[i].d_q);
        c->pc[i].d_recs = nullptr; c->pc[i].d_q = nullptr;
        for (int o = 0; o < 2; o++)
            for (int sg = 0; sg < 2; sg++) {
                if (c->pc[i].d_g_recs[o][sg]) dev_free(c->pc[i].d_g_recs[o][sg]);
                c->pc[i].d_g_recs[o][sg] = nullptr;
                c->pc[i].g_recs[o][sg].clear();
            }
        c->pc[i].recs.clear(); c->pc[i].q.clear();
    }
    void *ptrs[] = {c->d_prim, c->d_M, c->d_tile_table, c->d_tile_off, c->d_tile_I, c->d_runs, c->d_tiles, c->d_segs, c->d_wave_seg,
                    c->d_tile_present};
    for (void *p : ptrs) if (p) dev_free(p);
    c->d_tile_present = nullptr;
    c->d_prim = c->d_M = nullptr; c->d_tile_table = nullptr; c->d_tile_off = nullptr; c->d_tile_I = nullptr;
    c->d_runs = nullptr; c->d_tiles = nullptr; c->d_segs = nullptr; c->d_wave_seg = nullptr;
    c->eri_ready = false;
}

// Drop the resident tile store and the pair data of the last mi_eri_prepare (the store is parked for reuse, see TileArena).
// Used when the ranks of a sharded run agree on the direct mode although THIS rank's shard would have fitted.
extern "C" int mi_eri_release(mi_ctx *c)
{
    if (!c) return fail("mi_eri_release: null context");
    hipSetDevice(c->device);
    free_eri(c);
    return 0;
}

extern "C" void mi_ctx_destroy(mi_ctx *c)
{
    if (!c) return;
    hipSetDevice(c->device);
    free_eri(c);
    void *ptrs[] = {c->d_env, c->d_bas, c->d_atm, c->d_shell_ao, c->d_c2s, c->d_rys_cheb, c->d_herm_r, c->d_herm_w,
                    c->pair_classes[0].d_pairs, c->pair_classes[1].d_pairs,
                    c->d_Dpad, c->d_Jacc, c->d_Kacc, c->d_red, c->d_shell_xyz, c->d_xt_scratch, c->d_perm, c->d_iperm,
                    c->d_mDpad, c->d_mJacc, c->d_mKacc};
    for (void *p : ptrs) if (p) dev_free(p);
    // the large host vectors of the context (pair records and gradient matrices, tile directory: several hundred MB for
    // ibuprofen/def2-TZVP) are handed to the next context on this device instead of being unmapped here (~40 ms) and faulted
    // in again there: a geometry step replaces its context
    {
        HostStash &H = g_stash[c->device & 15];
        std::lock_guard<std::mutex> g(H.mu);
        if (c->h_M.capacity() > H.h_M.capacity()) H.h_M.swap(c->h_M);
        if (c->h_prim.capacity() > H.h_prim.capacity()) H.h_prim.swap(c->h_prim);
        if (c->tiles.capacity() > H.tiles.capacity()) H.tiles.swap(c->tiles);
        if (c->tile_off.capacity() > H.tile_off.capacity()) H.tile_off.swap(c->tile_off);
    }
    delete c;
}

extern "C" int mi_ctx_nao(const mi_ctx *c) { return c ? c->nao : -1; }

extern "C" int mi_set_option(mi_ctx *c, const char *key, double value)
{
    if (!c || !key) return fail("mi_set_option: null argument");
    std::string k(key);
    if (k == "runmax") c->opt_runmax = (int)value;           // takes effect at the next mi_eri_prepare
    else if (k == "omega") {                                  // takes effect at the next mi_eri_prepare
        if (!(value >= 0.0) || !std::isfinite(value)) return fail("mi_set_option: omega must be finite and >= 0");
        c->opt_omega = value;
    }
    else if (k == "jk_waves") c->opt_jk_waves = (int)value; // takes effect at the next mi_eri_prepare
    else if (k == "jk_nt") c->opt_jk_nt = (int)value;
    else if (k == "jk_pipe") c->opt_jk_pipe = (int)value;
    else if (k == "jk_dpp") c->opt_jk_dpp = (int)value;
    else if (k == "jk_kjlt") c->opt_jk_kjlt = (int)value;
    else if (k == "grad_live") c->opt_grad_live = (int)value;
    else if (k == "grad_rows") c->opt_grad_rows = (int)value;
    else if (k == "grad_rows_min") c->opt_grad_rows_min = (int)value;
    else if (k == "grad_rows_g32") g_rows_g32 = (int)value;
    else if (k == "jk_cache_mb") c->opt_jk_cache_mb = (int)value;
    else if (k == "jk_pair") c->opt_jk_pair = (int)value;
    else if (k == "jk_multi_batch") c->opt_jk_multi_batch = (int)value;
    else if (k == "sp2_direct") c->opt_sp2_direct = (int)value;
    else if (k == "vmat_wgs") c->opt_vmat_wgs = (int)value;
    else if (k == "vmat_xcd") c->opt_vmat_xcd = (int)value;
    else if (k == "tri_tiles") c->opt_tri_tiles = (int)value;       // takes effect at the next mi_eri_prepare
    else if (k == "ao_order") c->opt_ao_order = (int)value;         // takes effect at the next mi_eri_prepare
    else if (k == "ket_cluster") c->opt_ket_cluster = (int)value;   // takes effect at the next mi_eri_prepare
    else if (k == "xcd_map") c->opt_xcd_map = (int)value;
    else if (k == "prim_lds") c->opt_prim_lds = (int)value;
    else if (k == "task_table") c->opt_task_table = (int)value;
    else if (k == "eri_fused") c->opt_eri_fused = (int)value;
    else if (k == "rys_fine") c->opt_rys_fine = (int)value;
    else if (k == "df_batch_max") {
        if (!(value >= 0.0) || value > 2147483647.0) return fail("mi_set_option: df_batch_max must be in [0, 2^31)");
        c->opt_df_batch_max = (int)value;
    }
    else if (k == "vmat_fold_mt") c->opt_vmat_fold_mt = (int)value;
    else if (k == "work_mb") c->opt_work_mb = (int)value;
    else if (k == "grad_work_mb") c->opt_grad_work_mb = (int)value;
    else if (k == "rys_qpw_maxcomp") c->opt_rys_qpw_maxcomp = (int)value;
    else if (k == "rys_qpw_maxprim") c->opt_rys_qpw_maxprim = value;
    else if (k == "xf_qpw_max") c->opt_xf_qpw_max = (int)value;
    else if (k == "xf_mlds") c->opt_xf_mlds = (int)value;
    else if (k == "eri_tpq") c->opt_eri_tpq = (int)value;
    else if (k == "tpq_maxprim") c->opt_tpq_maxprim = value;
    else if (k == "tpq_min_tasks") c->opt_tpq_min_tasks = (int64_t)value;
    else if (k == "xf_mfma_min") c->opt_xf_mfma_min = (int)value;   // takes effect at the next mi_eri_prepare
    else if (k == "grad_dtol") c->opt_grad_dtol = value;
    else if (k == "grad_prefetch") c->opt_grad_prefetch = (int)value;   // takes effect at the next mi_eri_prepare
    else return fail("mi_set_option: unknown key '%s'", key);
    return 0;
}

// =================================================================================================
// One-electron integrals.
//
// The pieces below are the one body of the four kernel families that evaluate <m|1/r_C|n> or its attenuated twin
// <m|erf(zeta r_C)/r_C|n>: int1e_kernel (S, T, V, dipole), int1e_grad_kernel (section "Analytic nuclear gradient, one-electron
// part"), pcm_int_kernel and pcm_grad_kernel (section "C-PCM").  All are templates on the angular class <LA, LB>: every table is a
// fixed-size array indexed inside fully unrolled loops (registers, no per-thread blocks sized for the largest class), and a
// launch holds the shell pairs of ONE class from the context's class-sorted lists (mi_ctx::pair_classes).
// =================================================================================================
__device__ inline void cart_pow(int l, int idx, int &x, int &y, int &z)
{
    int n = 0;
    for (int lx = l; lx >= 0; lx--) {
        int cnt = l - lx + 1;
        if (idx < n + cnt) { x = lx; y = l - lx - (idx - n); z = l - x - y; return; }
        n += cnt;
    }
    x = y = z = 0;
}

__device__ inline int cart_exp(int l, int idx, int d)   // exponent of direction d of cartesian component idx of shell l
{
    int x = 0, y = 0, z = 0;
    cart_pow(l, idx, x, y, z);
    return d == 0 ? x : (d == 1 ? y : z);
}

// The basis as the one-electron, PCM and AO-value kernels read it: base of their argument structs.
struct BasisDev {
    const int32_t *atm, *bas;
    const double *env;
    const int *shell_ao;
    const double *c2s;
    int c2s_off[LMAX + 2];
    RysDev rys;
    int natm, nbas, nao;
};

static BasisDev basis_dev(const mi_ctx *c)
{
    BasisDev B;
    B.atm = c->d_atm; B.bas = c->d_bas; B.env = c->d_env; B.shell_ao = c->d_shell_ao; B.c2s = c->d_c2s;
    for (int i = 0; i <= LMAX + 1; i++) B.c2s_off[i] = c->c2s_off[i];
    B.rys = c->rys; B.natm = c->natm; B.nbas = c->nbas; B.nao = c->nao;
    return B;
}

// One primitive pair of the shells with `bas` rows bi, bj on centres ra, rb (AB = ra - rb).
struct PrimPair {
    double a, b, cc;   // exponents, product of the contraction coefficients (times whatever the caller folds in)
    double p, h, ex;   // a + b, 1 / 2p, exp(-a b / p |AB|^2)
    double PA[3], PB[3], P[3];
};

__device__ __forceinline__ PrimPair prim_pair(const double *env, const int32_t *bi, const int32_t *bj, int ip, int jp, const double *ra,
                                              const double *rb, const double (&AB)[3])
{
    PrimPair q;
    q.a = env[bi[5] + ip]; q.b = env[bj[5] + jp];
    q.cc = env[bi[6] + ip] * env[bj[6] + jp];
    q.p = q.a + q.b; q.h = 0.5 / q.p;
    q.ex = exp(-q.a * q.b / q.p * (AB[0] * AB[0] + AB[1] * AB[1] + AB[2] * AB[2]));
#pragma unroll
    for (int d = 0; d < 3; d++) {
        q.P[d] = (q.a * ra[d] + q.b * rb[d]) / q.p;
        q.PA[d] = q.P[d] - ra[d];
        q.PB[d] = q.P[d] - rb[d];
    }
    return q;
}

// 1-D attraction table gt[d][i][j], i + j < NI, of Rys root r of nr for the operator centred at C: vertical recurrence on the
// first shell, then the horizontal transfer with AB.  Returns prefactor x weight of the root.  ATTENUATED: erf(sqrt(eta) r)/r
// -- with theta = eta / (p + eta) the Boys argument and the root are scaled by theta and the prefactor by sqrt(theta);
// otherwise the plain nuclear formula (eta unused).
template <int LB, int NI, bool ATTENUATED>
__device__ __forceinline__ double attraction_table(double (&gt)[3][NI][LB + 1], const PrimPair &q, const double *C, double eta,
                                                   const double (&AB)[3], int nr, int r, const RysDev &rys)
{
    const double PC[3] = {q.P[0] - C[0], q.P[1] - C[1], q.P[2] - C[2]};
    const double r2 = PC[0] * PC[0] + PC[1] * PC[1] + PC[2] * PC[2];
    double x, pv, u;
    if constexpr (ATTENUATED) {
        const double theta = eta / (q.p + eta);
        x = q.p * theta * r2;
        pv = q.cc * q.ex * 2.0 * M_PI / q.p * sqrt(theta);
        u = rys_eval(rys, nr, r, x) * theta;
    } else {
        x = q.p * r2;
        pv = q.cc * q.ex * 2.0 * M_PI / q.p;
        u = rys_eval(rys, nr, r, x);
    }
    const double w = rys_eval(rys, nr, nr + r, x);
    const double b10 = (1.0 - u) * q.h;
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const double c00 = q.PA[d] - u * PC[d];
        gt[d][0][0] = 1.0;
#pragma unroll
        for (int i = 0; i + 1 < NI; i++) gt[d][i + 1][0] = c00 * gt[d][i][0] + (i > 0 ? i * b10 * gt[d][i > 0 ? i - 1 : 0][0] : 0.0);
#pragma unroll
        for (int j = 0; j < LB; j++)
#pragma unroll
            for (int i = 0; i < NI - j - 1; i++) gt[d][i][j + 1] = gt[d][i + 1][j] + AB[d] * gt[d][i][j];
    }
    return pv * w;
}

// acc[ia][ib] += f g_x g_y g_z: the cartesian block of one root
template <int LA, int LB, int NI>
__device__ __forceinline__ void attraction_accumulate(double *acc, const double (&gt)[3][NI][LB + 1], double f)
{
    constexpr int NCA = (LA + 1) * (LA + 2) / 2, NCB = (LB + 1) * (LB + 2) / 2;
#pragma unroll
    for (int ia = 0; ia < NCA; ia++)
#pragma unroll
        for (int ib = 0; ib < NCB; ib++)
            acc[ia * NCB + ib] += f * gt[0][cart_exp(LA, ia, 0)][cart_exp(LB, ib, 0)] * gt[1][cart_exp(LA, ia, 1)][cart_exp(LB, ib, 1)] *
                                  gt[2][cart_exp(LA, ia, 2)][cart_exp(LB, ib, 2)];
}

// gc[x] += f sum_{ia,ib} Dc[ia][ib] d/dA_x of the block of one root: d/dA_x acts on the 1-D factor as 2a g[i+1][j] - i g[i-1][j]
template <int LA, int LB, int NI>
__device__ __forceinline__ void attraction_bra_gradient(double (&gc)[3], const double (&gt)[3][NI][LB + 1], double f, double a, const double *Dc)
{
    constexpr int NCA = (LA + 1) * (LA + 2) / 2, NCB = (LB + 1) * (LB + 2) / 2;
#pragma unroll
    for (int ia = 0; ia < NCA; ia++)
#pragma unroll
        for (int ib = 0; ib < NCB; ib++) {
            double v0[3], vd[3];
#pragma unroll
            for (int d = 0; d < 3; d++) {
                const int i = cart_exp(LA, ia, d), j = cart_exp(LB, ib, d);
                v0[d] = gt[d][i][j];
                vd[d] = 2.0 * a * gt[d][i + 1][j] - (i > 0 ? i * gt[d][i > 0 ? i - 1 : 0][j] : 0.0);
            }
            const double dc = f * Dc[ia * NCB + ib];
            gc[0] += dc * vd[0] * v0[1] * v0[2];
            gc[1] += dc * v0[0] * vd[1] * v0[2];
            gc[2] += dc * v0[0] * v0[1] * vd[2];
        }
}

// Obara-Saika 1-D overlaps s[d][i][j], i <= LA + 1 (dipole, bra derivative), j <= LB + 2 (kinetic), without the prefactor
template <int LA, int LB>
__device__ __forceinline__ void overlap_table(double (&s)[3][LA + 2][LB + 3], const PrimPair &q)
{
#pragma unroll
    for (int d = 0; d < 3; d++) {
        s[d][0][0] = 1.0;
#pragma unroll
        for (int i = 0; i <= LA; i++) s[d][i + 1][0] = q.PA[d] * s[d][i][0] + (i > 0 ? i * q.h * s[d][i > 0 ? i - 1 : 0][0] : 0.0);
#pragma unroll
        for (int j = 0; j <= LB + 1; j++)
#pragma unroll
            for (int i = 0; i <= LA + 1; i++)
                s[d][i][j + 1] = q.PB[d] * s[d][i][j] + (i > 0 ? i * q.h * s[d][i > 0 ? i - 1 : 0][j] : 0.0) +
                                 (j > 0 ? j * q.h * s[d][i][j > 0 ? j - 1 : 0] : 0.0);
    }
}

// kinetic 1-D factor T(i, j) = -1/2 <i| d^2/dx^2 |j> from one direction's overlaps (b: exponent of the second shell)
template <int NA, int NB>
__device__ __forceinline__ double kinetic_1d(const double (&s)[NA][NB], int i, int j, double b)
{
    double t = -2.0 * b * (2 * j + 1) * s[i][j] + 4.0 * b * b * s[i][j + 2];
    if (j >= 2) t += j * (j - 1) * s[i][j >= 2 ? j - 2 : 0];
    return -0.5 * t;
}

// element (i, j) of the spherical block ca^T acc cb (ca, cb: cart -> sph tables of LA, LB)
template <int LA, int LB>
__device__ __forceinline__ double block_to_spherical(const double *acc, const double *ca, const double *cb, int i, int j)
{
    constexpr int NCA = (LA + 1) * (LA + 2) / 2, NCB = (LB + 1) * (LB + 2) / 2, NSA = 2 * LA + 1, NSB = 2 * LB + 1;
    double v = 0.0;
#pragma unroll
    for (int ia = 0; ia < NCA; ia++) {
        double t = 0.0;
#pragma unroll
        for (int ib = 0; ib < NCB; ib++) t += acc[ia * NCB + ib] * cb[ib * NSB + j];
        v += ca[ia * NSA + i] * t;
    }
    return v;
}

// element (ia, ib) of ca D_block cb^T: the spherical density block at AOs (ao_i.., ao_j..) back-transformed to cartesian components
template <int LA, int LB>
__device__ __forceinline__ double density_block_to_cartesian(const double *D, int nao, int ao_i, int ao_j, const double *ca, const double *cb,
                                                             int ia, int ib)
{
    constexpr int NSA = 2 * LA + 1, NSB = 2 * LB + 1;
    double s = 0.0;
    for (int i = 0; i < NSA; i++) {
        double t = 0.0;
        for (int j = 0; j < NSB; j++) t += D[(size_t)(ao_i + i) * nao + ao_j + j] * cb[ib * NSB + j];
        s += ca[ia * NSA + i] * t;
    }
    return s;
}

// One launch of KERNEL<la, lb> per non-empty angular class of the context's pair list: launch(la, lb, first, count) gets the
// class as two std::integral_constant and its rows of the list.  blocks_per_pair: workgroups a launch spends per pair in grid.x.
template <bool ORDERED, class F>
static int launch_pair_classes(const mi_ctx *c, int64_t blocks_per_pair, const char *who, F launch)
{
    const mi_ctx::PairClasses &pc = c->pair_classes[ORDERED];
    if ((int64_t)pc.start[16] * blocks_per_pair >= (int64_t)1 << 31)
        return fail("%s: %d shell pairs x %lld point blocks exceed one launch", who, pc.start[16], (long long)blocks_per_pair);
#define PAIR_CLASS(a, b)                                                                                                \
    if constexpr (ORDERED || (a) >= (b)) {                                                                              \
        const int first = pc.start[(a) * 4 + (b)], count = pc.start[(a) * 4 + (b) + 1] - first;                         \
        if (count > 0) launch(std::integral_constant<int, a>{}, std::integral_constant<int, b>{}, first, count);        \
    }
    PAIR_CLASS(0, 0) PAIR_CLASS(0, 1) PAIR_CLASS(0, 2) PAIR_CLASS(0, 3) PAIR_CLASS(1, 0) PAIR_CLASS(1, 1) PAIR_CLASS(1, 2) PAIR_CLASS(1, 3)
    PAIR_CLASS(2, 0) PAIR_CLASS(2, 1) PAIR_CLASS(2, 2) PAIR_CLASS(2, 3) PAIR_CLASS(3, 0) PAIR_CLASS(3, 1) PAIR_CLASS(3, 2) PAIR_CLASS(3, 3)
#undef PAIR_CLASS
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail("%s: launch failed: %s", who, hipGetErrorString(e));
    return 0;
}

struct Int1eArgs : BasisDev {
    const int *pairs;   // [npair][2] shell pairs of the launch's class, l of the first >= l of the second
    int npair;
    double *S, *T, *V, *dip;
    double org[3];
};

// One thread per shell pair.  grid.y = natm + 1: slice y < natm adds the nuclear-attraction contribution of nucleus y (FP64
// atomics into a zeroed V: natm-fold more parallelism for the only part that scales with the number of atoms), slice y == natm
// writes S, T and the dipole blocks.  The pair's first shell has the higher l, not necessarily the higher index: block (i, j) and
// its transpose are stored, and the dipole operator is raised on the first shell's centre.
template <int LA, int LB>
__global__ __launch_bounds__(64) void int1e_kernel(Int1eArgs A)
{
    constexpr int NCA = (LA + 1) * (LA + 2) / 2, NCB = (LB + 1) * (LB + 2) / 2, NSA = 2 * LA + 1, NSB = 2 * LB + 1;
    constexpr int NR = (LA + LB) / 2 + 1, NI = LA + LB + 1;
    const int pid = blockIdx.x * blockDim.x + threadIdx.x;
    if (pid >= A.npair) return;
    const int vatom = (int)blockIdx.y < A.natm ? (int)blockIdx.y : -1; // -1: the S/T/dipole slice
    if (vatom >= 0 && (A.V == nullptr || A.atm[vatom * ATM_SLOTS + 0] == 0)) return;
    const int ish = A.pairs[2 * pid], jsh = A.pairs[2 * pid + 1];
    const int32_t *bi = A.bas + ish * BAS_SLOTS, *bj = A.bas + jsh * BAS_SLOTS;
    const double *ra = A.env + A.atm[bi[0] * ATM_SLOTS + 1], *rb = A.env + A.atm[bj[0] * ATM_SLOTS + 1];
    const double AB[3] = {ra[0] - rb[0], ra[1] - rb[1], ra[2] - rb[2]};
    const double *ca = A.c2s + A.c2s_off[LA], *cb = A.c2s + A.c2s_off[LB];
    const int ao_i = A.shell_ao[ish], ao_j = A.shell_ao[jsh];
    if (vatom >= 0) {
        const double Z = A.atm[vatom * ATM_SLOTS + 0];
        const double *C = A.env + A.atm[vatom * ATM_SLOTS + 1];
        double acc[NCA * NCB];
#pragma unroll
        for (int k = 0; k < NCA * NCB; k++) acc[k] = 0.0;
        for (int ip = 0; ip < bi[2]; ip++)
            for (int jp = 0; jp < bj[2]; jp++) {
                const PrimPair q = prim_pair(A.env, bi, bj, ip, jp, ra, rb, AB);
#pragma unroll
                for (int r = 0; r < NR; r++) {
                    double gt[3][NI][LB + 1];
                    const double f = attraction_table<LB, NI, false>(gt, q, C, 0.0, AB, NR, r, A.rys);
                    attraction_accumulate<LA, LB>(acc, gt, -Z * f);
                }
            }
        // one nucleus' share: accumulate (the diagonal shell pair visits (i,j) and (j,i) itself)
        for (int i = 0; i < NSA; i++)
            for (int j = 0; j < NSB; j++) {
                const double v = block_to_spherical<LA, LB>(acc, ca, cb, i, j);
                atomicAdd(&A.V[(size_t)(ao_i + i) * A.nao + ao_j + j], v);
                if (ish != jsh) atomicAdd(&A.V[(size_t)(ao_j + j) * A.nao + ao_i + i], v);
            }
        return;
    }
    double blk[5][NCA * NCB];   // cartesian blocks of S, T, x, y, z
#pragma unroll
    for (int m = 0; m < 5; m++)
#pragma unroll
        for (int k = 0; k < NCA * NCB; k++) blk[m][k] = 0.0;
    for (int ip = 0; ip < bi[2]; ip++)
        for (int jp = 0; jp < bj[2]; jp++) {
            const PrimPair q = prim_pair(A.env, bi, bj, ip, jp, ra, rb, AB);
            double s[3][LA + 2][LB + 3];
            overlap_table<LA, LB>(s, q);
            const double pref = q.cc * q.ex * pow(M_PI / q.p, 1.5);
#pragma unroll
            for (int ia = 0; ia < NCA; ia++)
#pragma unroll
                for (int ib = 0; ib < NCB; ib++) {
                    double s1[3], t1[3], x1[3];
#pragma unroll
                    for (int d = 0; d < 3; d++) {
                        const int i = cart_exp(LA, ia, d), j = cart_exp(LB, ib, d);
                        s1[d] = s[d][i][j];
                        t1[d] = kinetic_1d(s[d], i, j, q.b);
                        x1[d] = s[d][i + 1][j] + (ra[d] - A.org[d]) * s1[d];
                    }
                    const int k = ia * NCB + ib;
                    blk[0][k] += pref * s1[0] * s1[1] * s1[2];
                    blk[1][k] += pref * (t1[0] * s1[1] * s1[2] + s1[0] * t1[1] * s1[2] + s1[0] * s1[1] * t1[2]);
                    blk[2][k] += pref * x1[0] * s1[1] * s1[2];
                    blk[3][k] += pref * s1[0] * x1[1] * s1[2];
                    blk[4][k] += pref * s1[0] * s1[1] * x1[2];
                }
        }
    // cart -> sph and store both triangles
    double *outs[5] = {A.S, A.T, A.dip, A.dip ? A.dip + (size_t)A.nao * A.nao : nullptr, A.dip ? A.dip + 2 * (size_t)A.nao * A.nao : nullptr};
#pragma unroll
    for (int m = 0; m < 5; m++) {
        if (!outs[m]) continue;
        for (int i = 0; i < NSA; i++)
            for (int j = 0; j < NSB; j++) {
                const double v = block_to_spherical<LA, LB>(blk[m], ca, cb, i, j);
                outs[m][(size_t)(ao_i + i) * A.nao + ao_j + j] = v;
                outs[m][(size_t)(ao_j + j) * A.nao + ao_i + i] = v;
            }
    }
}

// orbital paths (one-electron integrals, AO values on the grid, resident ERI tiles and their gradients) stop at f shells
static int check_orbital_lmax(const mi_ctx *c, const char *who)
{
    for (const ShellH &sh : c->shells)
        if (sh.l > LMAX_1E) return fail("%s: shell with l = %d (orbital shells stop at l = %d; g shells are for auxiliary contexts)", who, sh.l, LMAX_1E);
    return 0;
}

extern "C" int mi_int1e(mi_ctx *c, double *d_S, double *d_T, double *d_V, double *d_dip, const double *origin, void *stream)
{
    if (c && check_orbital_lmax(c, "mi_int1e")) return -1;
    if (!c) return fail("mi_int1e: null context");
    HIPCHK(hipSetDevice(c->device));
    Int1eArgs A{basis_dev(c)};
    A.S = d_S; A.T = d_T; A.V = d_V; A.dip = d_dip;
    for (int d = 0; d < 3; d++) A.org[d] = origin ? origin[d] : 0.0;
    if (d_V) HIPCHK(hipMemsetAsync(d_V, 0, sizeof(double) * (size_t)c->nao * c->nao, (hipStream_t)stream));
    return launch_pair_classes<false>(c, 1, "mi_int1e", [&](auto la, auto lb, int first, int count) {
        A.pairs = c->pair_classes[0].d_pairs + 2 * first;
        A.npair = count;
        hipLaunchKernelGGL((int1e_kernel<decltype(la)::value, decltype(lb)::value>), dim3((count + 63) / 64, c->natm + 1), dim3(64), 0,
                           (hipStream_t)stream, A);
    });
}

// Upper bound of |G| = |D_ab D_cd - hyb/4 (D_ac D_bd + D_ad D_bc)| over the AO quadruples of a shell quartet.
// qmax (pair mode, mi_grad_eri_pairs): G has the extra term sum_k s_k Q^k_ab Q^k_cd, bounded by qmax_ab qmax_cd with
// qmax_ab = sqrt(sum_k |s_k| max_ab |Q^k|^2) (Cauchy-Schwarz over k).
// xmax (exchange-pair mode, mi_grad_eri_xpairs): G has the extra term sum_m t_m (R^m_ac R^m_bd + R^m_ad R^m_bc), bounded by
// xmax_ac xmax_bd + xmax_ad xmax_bc with xmax_ab = sqrt(sum_m |t_m| max_ab |R^m|^2) (|R^m| of the block and of its transpose).
__device__ inline double quartet_density_bound(const double *dmax, int nb, int a, int b, int c, int d, double hyb, const double *qmax, const double *xmax)
{
    double coul = dmax[a * nb + b] * dmax[c * nb + d];
    double exch = dmax[a * nb + c] * dmax[b * nb + d] + dmax[a * nb + d] * dmax[b * nb + c];
    double pairs = qmax ? qmax[a * nb + b] * qmax[c * nb + d] : 0.0;
    if (xmax) pairs += xmax[a * nb + c] * xmax[b * nb + d] + xmax[a * nb + d] * xmax[b * nb + c];
    return coul + 0.25 * hyb * exch + pairs;
}

// Pair mode of the gradient (mi_grad_eri_pairs): the two-particle density has the extra term sum_k s_k Q^k_ab Q^k_cd.  The Q^k
// are kept as P[(a * ld + b) * K + k] = sqrt|s_k| Q^k_ab (padded tile order like D, k fastest: one AO pair's K values are one
// contiguous run), the `npos` positive s_k first, so the term is a dot product of two runs with one change of sign.
struct PairTerm {
    const double *P;   // nullptr: no pair term
    int K, npos;
};
__device__ inline double pair_term(const PairTerm &T, size_t ab, size_t cd)
{
    const double *x = T.P + ab * T.K, *y = T.P + cd * T.K;
    double pos = 0.0, neg = 0.0;
    for (int k = 0; k < T.npos; k++) pos = fma(x[k], y[k], pos);
    for (int k = T.npos; k < T.K; k++) neg = fma(x[k], y[k], neg);
    return pos - neg;
}
// Exchange-pair mode (mi_grad_eri_xpairs): the extra term sum_m t_m (R^m_ik R^m_jl + R^m_il R^m_jk), the R^m kept like the Q^k
// (sqrt|t_m| R^m, m fastest, positive t_m first).  (i, j) is one pair of the quartet and (k, l) the other: every factor is read
// as [index of the (i, j) pair][index of the (k, l) pair], so for an antisymmetric R^m exchanging the two pairs changes the sign
// of both factors of a product and exchanging i, j or k, l exchanges the two products -- the term has the 8-fold symmetry of G.
__device__ inline double xpair_term(const PairTerm &T, size_t ik, size_t jl, size_t il, size_t jk)
{
    const double *a = T.P + ik * T.K, *b = T.P + jl * T.K, *c = T.P + il * T.K, *d = T.P + jk * T.K;
    double pos = 0.0, neg = 0.0;
    for (int m = 0; m < T.npos; m++) pos = fma(a[m], b[m], fma(c[m], d[m], pos));
    for (int m = T.npos; m < T.K; m++) neg = fma(a[m], b[m], fma(c[m], d[m], neg));
    return pos - neg;
}

// The two-particle density of one derivative quartet, the ONE place its element formula lives (gradient kernels
// eri_grad_contract, eri_grad_rows_kernel, eri_tpq_grad_kernel):
//   G_ijkl = D_ij D_kl - hyb/4 (D_ik D_jl + D_il D_jk [+ M_ik M_jl + M_il M_jk]) [+ pair_term(pt)] [+ xpair_term(xt)]
// Which optional terms are compiled in is the template argument GradTerms of those kernels, chosen once on the host
// (with_grad_terms); XPAIRS includes the pair term (pt.K may be 0).
enum class GradTerms { PLAIN, PAIRS, XPAIRS };
struct QuartetDensity {
    const double *D, *Dm;   // padded total density; padded spin density Da - Db (UHF/UKS) or nullptr
    int ld;
    double hyb;
    PairTerm pt;            // pair mode: G += sum_k s_k Q^k_ij Q^k_kl
    PairTerm xt;            // exchange-pair mode: G += sum_m t_m (R^m_ik R^m_jl + R^m_il R^m_jk)
    template <GradTerms T>
    __device__ double element(int i, int j, int k, int l) const
    {
        double ex = D[(size_t)i * ld + k] * D[(size_t)j * ld + l] + D[(size_t)i * ld + l] * D[(size_t)j * ld + k];
        if (Dm) // sum_s Ds x Ds = (D x D + M x M) / 2
            ex += Dm[(size_t)i * ld + k] * Dm[(size_t)j * ld + l] + Dm[(size_t)i * ld + l] * Dm[(size_t)j * ld + k];
        double gv = D[(size_t)i * ld + j] * D[(size_t)k * ld + l] - 0.25 * hyb * ex;
        if (T != GradTerms::PLAIN) gv += pair_term(pt, (size_t)i * ld + j, (size_t)k * ld + l);
        if (T == GradTerms::XPAIRS) gv += xpair_term(xt, (size_t)i * ld + k, (size_t)j * ld + l, (size_t)i * ld + l, (size_t)j * ld + k);
        return gv;
    }
};
// host: f(std::integral_constant<GradTerms, ...>) for the terms that `d` carries -- the one mode dispatch of the gradient launches
template <class F>
static int with_grad_terms(const QuartetDensity &d, F &&f)
{
    if (d.xt.P) return f(std::integral_constant<GradTerms, GradTerms::XPAIRS>{});
    if (d.pt.P) return f(std::integral_constant<GradTerms, GradTerms::PAIRS>{});
    return f(std::integral_constant<GradTerms, GradTerms::PLAIN>{});
}

// Density-weighted Schwarz screening of the derivative quartets: q_ab q_cd max|G| < dtol skips the quartet (dmax == nullptr:
// off -- the SCF's ERI evaluation, or a list of live quartets that is already screened).
struct QuartetScreen {
    const double *q_bra, *q_ket, *dmax; // Schwarz factors of the two pair lists; max |D| per shell pair [nbas_d][nbas_d]
    const double *qmax, *xmax;          // pair / exchange-pair mode: see quartet_density_bound (nullptr otherwise)
    int nbas_d;
    double dtol, hyb;
    // (ib, ik) index q_bra / q_ket; a, b | c, d are the shells of the two pairs
    __device__ bool negligible(int ib, int ik, int a, int b, int c, int d) const
    {
        return dmax && q_bra[ib] * q_ket[ik] * quartet_density_bound(dmax, nbas_d, a, b, c, d, hyb, qmax, xmax) < dtol;
    }
};

// =================================================================================================
// ERI generation, kernel 1: contracted [e0|f0] integrals by Rys quadrature.
//
// One 64-lane wave per shell quartet.  Per batch of PB primitive quartets:
//   phase R  lanes <-> (primitive quartet, root-or-weight function): Chebyshev evaluation -> LDS
//   phase A  lanes <-> (primitive quartet, root, direction): 2-D vertical recurrence table
//            T[n][m], n <= la+lb, m <= lc+ld  -> LDS
//   phase C  lanes <-> output components (e,f): sum over slots of Tx*Ty*Tz, accumulators in VGPRs
// =================================================================================================
struct TaskIdx { int ib, ik; };   // (bra, ket) of one task (get_task)
struct EriArgs {
    const PairRec *bra, *ket;
    const double *prim;
    const int64_t *prefix;   // [nbra+1] cumulative task counts
    int nbra;
    int64_t t0, ntask;       // this launch covers tasks [t0, t0+ntask)
    int la, lb, lc, ld;
    int nmax, mmax, nroots, tsz; // tsz = (nmax+1)*(mmax+1)
    int ncomp, PB;
    const uint32_t *comp;    // [ncomp] packed ix | iy<<10 | iz<<20
    double *work;            // [ntask][ncomp]
    RysDev rys;
    int diag;                // 1: Schwarz mode, ket == bra and task b -> (b,b)
    int swap;                // 1: the task's (bra index, ket index) address (ket[], bra[]) instead
    const int32_t *own_table; // non-null on a sharded context: skip quartets none of whose tiles live on this rank
    int ni, nj, nk, nl;       // spherical shell sizes (for the ownership test)
    QuartetScreen scr;        // scr.q_bra / scr.q_ket: Schwarz factors (qtol); the rest is the gradient's screening (dmax == nullptr: off)
    // host side only (kernel choice): primitive-pair statistics of the shared (bra) and the varying (ket) pair list
    double h_shared_np, h_vary_mean, h_vary_max4;
    const TaskIdx *tasks;    // non-null: (bra, ket) per task, precomputed (get_task)
    int prim_lds;            // > 0: stage the primitive-pair records of the quartet in LDS (room for this many records per quartet)
    double qtol;             // > 0: skip tasks with q_bra q_ket < qtol (kets of a surviving cluster that fail the Schwarz test themselves)
    unsigned xcd;            // > 0: XCD-aware block map with chunks of this many blocks (xcd_block), grid rounded up to 8 * xcd
    double omega;            // > 0: erf(omega r12)/r12 integrals (long-range store, rys_attenuate); 0: full Coulomb
};

// Long-range (erf-attenuated) Rys quadrature: with theta = omega^2 / (omega^2 + rho), rho = p q / (p + q), the integrals of
// erf(omega r12)/r12 are those of 1/r12 with the Rys argument theta x, the roots u theta and the weights (prefactor) sqrt(theta)
// -- the substitution of the PCM kernels (pcm_eval).  `f` < n is a root function, f >= n a weight function.  Called only
// under a uniform `omega > 0` branch, so the full-Coulomb path keeps its instruction sequence.
__device__ inline double rys_attenuate(const RysDev &R, int n, int f, double rho, double x, double omega)
{
    const double w2 = omega * omega, th = w2 / (w2 + rho);
    const double v = rys_eval(R, n, f, x * th);
    return f < n ? v * th : v * sqrt(th);
}

// Block index -> position in the task order such that `C` consecutive positions run on ONE XCD (blocks b and b + 8 share an
// XCD under the observed round-robin placement; speed only, never correctness): the pieces of a tile line written by
// neighbouring tasks then meet in one L2.  Chunks alternate over the XCDs, so the load stays balanced along the task list.
// The grid must be a multiple of 8 C (eri_grid); positions beyond the task count idle.
__device__ inline unsigned xcd_block(unsigned b, unsigned C)
{
    if (C == 0u) return b;
    const unsigned x = b & 7u, r = b >> 3;
    return ((r / C) * 8u + x) * C + (r % C);
}
static inline unsigned eri_grid(int64_t nblocks, unsigned C)
{
    if (C == 0u) return (unsigned)nblocks;
    const int64_t m = 8 * (int64_t)C;
    return (unsigned)((nblocks + m - 1) / m * m);
}

// Task t of a class pair -> (bra pair index, ket index).  `prefix` holds the nbra+1 cumulative task counts followed by
// a coarse index (one entry per 1024 tasks: the bra index of task g*1024, see append_coarse_index), so the search
// touches two neighbouring coarse entries and then only the few prefix entries between them.
__device__ inline void find_task(const int64_t *prefix, int nbra, int64_t t, int &ib, int &ik)
{
    const int64_t *coarse = prefix + nbra + 1;
    const int64_t g = t >> 10;
    int lo = (int)coarse[g], hi = min((int)coarse[g + 1] + 1, nbra); // prefix[lo] <= t < prefix[hi]
    while (hi - lo > 1) {
        int mid = (lo + hi) >> 1;
        if (prefix[mid] <= t) lo = mid; else hi = mid;
    }
    ib = lo;
    ik = (int)(t - prefix[lo]);
}

// (bra, ket) of every task of a class pair, written once (fill_tasks_kernel) when several launches walk the same task list --
// the Rys and transform launches of the evaluation, the 3 permutations x 3 launches of the gradient: one coalesced 8-byte load
// per quartet instead of the two or three DEPENDENT global loads of find_task (~2 us of a ~10 us quartet in those latency-
// bound kernels).
__device__ inline void get_task(const TaskIdx *tasks, const int64_t *prefix, int nbra, int64_t t, int &ib, int &ik)
{
    if (tasks) { const TaskIdx q = tasks[t]; ib = q.ib; ik = q.ik; }
    else find_task(prefix, nbra, t, ib, ik);
}
__global__ __launch_bounds__(256) void fill_tasks_kernel(const int64_t *prefix, int nbra, int64_t ntask, TaskIdx *out)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= ntask) return;
    int ib, ik;
    find_task(prefix, nbra, t, ib, ik);
    out[t] = TaskIdx{ib, ik};
}

// Gradient, density-weighted screening: the (bra, ket) list of the LIVE quartets of a class pair, in task order (round 3).  The
// bound is symmetric in the roles of the four shells, so one list serves the three permutations x three launches of the class:
// before, every launch started a wave per Schwarz-surviving quartet and the dead ones (q_ab q_cd max|G| < grad_dtol) left after
// decoding their task and reading two pair records, two Schwarz factors and six density maxima.
struct LiveArgs {
    const PairRec *bra, *ket;
    const int64_t *prefix;
    int nbra;
    int64_t ntask;
    QuartetScreen scr;
};
__device__ inline bool task_is_live(const LiveArgs &A, int64_t t, int &ib, int &ik)
{
    find_task(A.prefix, A.nbra, t, ib, ik);
    return !A.scr.negligible(ib, ik, A.bra[ib].sh_i, A.bra[ib].sh_j, A.ket[ik].sh_i, A.ket[ik].sh_j);
}
__global__ __launch_bounds__(256) void live_count_kernel(LiveArgs A, int *block_counts)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int ib, ik;
    const bool live = t < A.ntask && task_is_live(A, t, ib, ik);
    const int n = __syncthreads_count(live);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = n;
}
// exclusive prefix sum of `n` block counts by ONE workgroup (n <= a few 1e5); offsets[n] = total
__global__ __launch_bounds__(1024) void live_scan_kernel(const int *counts, int n, int64_t *offsets)
{
    __shared__ int64_t part[1024];
    __shared__ int64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < n; base += 1024) {
        const int idx = base + threadIdx.x;
        const int64_t v = idx < n ? counts[idx] : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {      // Hillis-Steele inclusive scan
            const int64_t add = threadIdx.x >= off ? part[threadIdx.x - off] : 0;
            __syncthreads();
            part[threadIdx.x] += add;
            __syncthreads();
        }
        if (idx < n) offsets[idx] = carry + part[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry += part[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) offsets[n] = carry;
}
__global__ __launch_bounds__(256) void live_fill_kernel(LiveArgs A, const int64_t *offsets, TaskIdx *out)
{
    __shared__ int wave_base[4];
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int ib = 0, ik = 0;
    const bool live = t < A.ntask && task_is_live(A, t, ib, ik);
    const unsigned long long m = __ballot(live);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_base[wave] = __popcll(m);
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; w++) base += wave_base[w];
    if (live) out[offsets[blockIdx.x] + base + __popcll(m & ((1ull << lane) - 1ull))] = TaskIdx{ib, ik};
}

// Does any AO quadruple of the shell quartet land in a tile that is resident on this rank?  (<= 16 block
// combinations; every symmetry image of a quadruple maps to the same canonical tile.)  Corner c of the quartet's block ranges:
// bit 0 .. 3 picks the last instead of the first block of shell i, j, k, l.
__device__ inline bool block_corner_resident(const int32_t *table, int corner, int ao_i, int ni, int ao_j, int nj, int ao_k, int nk,
                                             int ao_l, int nl)
{
    int I = (corner & 1) ? (ao_i + ni - 1) >> 3 : ao_i >> 3;
    int J = (corner & 2) ? (ao_j + nj - 1) >> 3 : ao_j >> 3;
    int K = (corner & 4) ? (ao_k + nk - 1) >> 3 : ao_k >> 3;
    int L = (corner & 8) ? (ao_l + nl - 1) >> 3 : ao_l >> 3;
    int hi = max(I, J), lo = min(I, J), bij = hi * (hi + 1) / 2 + lo;
    hi = max(K, L); lo = min(K, L);
    int bkl = hi * (hi + 1) / 2 + lo;
    int bmax = max(bij, bkl), bmin = min(bij, bkl);
    return table[(size_t)bmax * (bmax + 1) / 2 + bmin] >= 0;
}
// one thread looks at all 16 corners (thread-per-quartet kernels) ...
__device__ inline bool quartet_has_resident_tile_thread(const int32_t *table, int ao_i, int ni, int ao_j, int nj, int ao_k, int nk, int ao_l, int nl)
{
    bool hit = false;
    for (int q = 0; q < 16; q++) hit = hit || block_corner_resident(table, q, ao_i, ni, ao_j, nj, ao_k, nk, ao_l, nl);
    return hit;
}
// ... or 16 lanes one each (wave-per-quartet kernels)
__device__ inline bool quartet_has_resident_tile(const int32_t *table, int ao_i, int ni, int ao_j, int nj, int ao_k, int nk,
                                                 int ao_l, int nl, int lane, int gsz = 64, int grp = 0)
{
    // `lane` is the lane inside a group of `gsz` (>= 16) lanes working on this quartet; groups vote separately
    const bool hit = lane < 16 && block_corner_resident(table, lane, ao_i, ni, ao_j, nj, ao_k, nk, ao_l, nl);
    const unsigned long long votes = __ballot(hit);
    const unsigned long long gmask = (gsz >= 64 ? ~0ull : ((1ull << gsz) - 1ull) << (gsz * grp));
    return (votes & gmask) != 0ull;
}

// ---- the Rys phases of the wave-per-quartet kernels (eri_rys_kernel, the fused kernel's first half, eri_grad_rows_kernel) ----
// LDS of one quartet's Rys phases: T0 [PB n][3][tsz] recurrence tables, then rw [PB][2 n] roots and weights; what a kernel keeps
// behind them (staged primitive records, the row kernel's matrices) starts at doubles().  Kernels and host launches size from it.
struct RysLds {
    int PB, n, tsz;
    __host__ __device__ size_t rw() const { return (size_t)PB * n * 3 * tsz; }
    __host__ __device__ size_t doubles() const { return rw() + (size_t)PB * 2 * n; }
};

// prim_b / prim_k: the primitive-pair records of the two pairs; primitive quartet pq = ip * ncd + jp.
// ONE_TRIP: the caller's batch fits the group (npq * 3 n <= GSZ, as PB = GSZ / (3 n) guarantees), so a lane has at most one item and
// the loop is a guard; the 16-lane groups of eri_rys_kernel would otherwise diverge on the trip count (measured 5-12 % on their
// classes).  The row kernel keeps its strided loop.
// phase R: roots and weights of the primitive quartets pq0 .. pq0 + npq - 1, one (primitive quartet, function) per lane of the group
template <int GSZ, bool ONE_TRIP>
__device__ __forceinline__ void rys_phase_roots(const RysDev &rys, double omega, int n, const double *prim_b, const double *prim_k, int ncd, int pq0,
                                                int npq, int lane, double *rw)
{
    for (int idx = lane; idx < npq * 2 * n; idx += GSZ) {
        const int pql = idx / (2 * n), f = idx - pql * 2 * n;
        const int pq = pq0 + pql, ip = pq / ncd, jp = pq - ip * ncd;
        const double *b = prim_b + (size_t)ip * 8, *k = prim_k + (size_t)jp * 8;
        const double p = b[0], q = k[0];
        const double dx = b[1] - k[1], dy = b[2] - k[2], dz = b[3] - k[3];
        const double rho = p * q / (p + q), x = rho * (dx * dx + dy * dy + dz * dz);
        if (omega > 0.0) rw[idx] = rys_attenuate(rys, n, f, rho, x, omega);
        else rw[idx] = rys_eval(rys, n, f, x);
        if (ONE_TRIP) break;
    }
}
// phase A: the 2-D vertical recurrence tables T[i][m], i <= nmax, m <= mmax, one (primitive quartet, root, direction) per lane;
// the z table carries the weight and the prefactor 2 pi^(5/2) K_ab K_cd / (p q sqrt(p + q))
template <int GSZ, bool ONE_TRIP>
__device__ __forceinline__ void rys_phase_tables(int n, int nmax, int mmax, int tsz, const double *prim_b, const double *prim_k, int ncd, int pq0,
                                                 int npq, int lane, const double *rw, double *T0)
{
    const int M1 = mmax + 1;
    for (int idx = lane; idx < npq * n * 3; idx += GSZ) {
        const int pql = idx / (3 * n), rem = idx - pql * 3 * n, r = rem / 3, d = rem - r * 3;
        const int pq = pq0 + pql, ip = pq / ncd, jp = pq - ip * ncd;
        const double *b = prim_b + (size_t)ip * 8, *k = prim_k + (size_t)jp * 8;
        const double p = b[0], q = k[0], pq1 = 1.0 / (p + q);
        const double u = rw[pql * 2 * n + r];
        const double PQd = b[1 + d] - k[1 + d];
        const double b00 = 0.5 * u * pq1, b10 = 0.5 / p * (1.0 - u * q * pq1), b01 = 0.5 / q * (1.0 - u * p * pq1);
        const double c00 = b[4 + d] - u * q * pq1 * PQd, c01 = k[4 + d] + u * p * pq1 * PQd;
        double *T = T0 + (size_t)idx * tsz;
        double t00 = 1.0;
        if (d == 2) t00 = rw[pql * 2 * n + n + r] * b[7] * k[7] * 34.986836655249725 /* 2 pi^2.5 */ * pq1 * sqrt(p + q) / (p * q);
        T[0] = t00;
        double tm = 0.0, tc = t00;
        for (int i = 0; i < nmax; i++) {
            const double tn = c00 * tc + i * b10 * tm;
            T[(i + 1) * M1] = tn;
            tm = tc; tc = tn;
        }
        for (int m = 0; m < mmax; m++)
            for (int i = 0; i <= nmax; i++) {
                double v = c01 * T[i * M1 + m];
                if (m > 0) v += m * b01 * T[i * M1 + m - 1];
                if (i > 0) v += i * b00 * T[(i - 1) * M1 + m];
                T[i * M1 + m + 1] = v;
            }
        if (ONE_TRIP) break;
    }
}

// The Rys phases of ONE quartet on a group of GSZ lanes: per batch of PB primitive quartets phase R, phase A, then phase C, the
// component products through the packed `comp` words, MAXC components per lane in registers.  nPQ: primitive quartets of this
// group's quartet (0: the group has none and only keeps the barriers); nPQ_all: the largest nPQ of the wave, the uniform trip
// count.  lds: the group's RysLds block.  store(c, v) receives component c of the contracted [e0|f0] block.
template <int MAXC, int GSZ, class Store>
__device__ __forceinline__ void rys_quartet_body(const EriArgs &A, const double *prim_b, const double *prim_k, int ncd, int nPQ, int nPQ_all, int lane, double *lds, Store store)
{
    const int n = A.nroots, tsz = A.tsz, PB = A.PB;
    double *T0 = lds, *rw = lds + RysLds{PB, n, tsz}.rw();
    for (int c0 = 0; c0 < A.ncomp; c0 += GSZ * MAXC) {
        double acc[MAXC];
        uint32_t idx[MAXC];
#pragma unroll
        for (int ci = 0; ci < MAXC; ci++) {
            acc[ci] = 0.0;
            const int c = c0 + ci * GSZ + lane;
            idx[ci] = (c < A.ncomp) ? A.comp[c] : 0xFFFFFFFFu;
        }
        for (int pq0 = 0; pq0 < nPQ_all; pq0 += PB) {
            const int npq = GSZ == 64 ? min(PB, nPQ - pq0) : max(0, min(PB, nPQ - pq0));
            rys_phase_roots<GSZ, true>(A.rys, A.omega, n, prim_b, prim_k, ncd, pq0, npq, lane, rw);
            __syncthreads();
            rys_phase_tables<GSZ, true>(n, A.nmax, A.mmax, tsz, prim_b, prim_k, ncd, pq0, npq, lane, rw, T0);
            __syncthreads();
            const int nslot = npq * n;
            for (int s = 0; s < nslot; s++) {
                const double *Tx = T0 + (size_t)s * 3 * tsz, *Ty = Tx + tsz, *Tz = Ty + tsz;
#pragma unroll
                for (int ci = 0; ci < MAXC; ci++) {
                    const uint32_t w = idx[ci];
                    if (w != 0xFFFFFFFFu) acc[ci] += Tx[w & 1023u] * Ty[(w >> 10) & 1023u] * Tz[(w >> 20) & 1023u];
                }
            }
            __syncthreads();
        }
        if (nPQ > 0) {
#pragma unroll
            for (int ci = 0; ci < MAXC; ci++) {
                const int c = c0 + ci * GSZ + lane;
                if (c < A.ncomp) store(c, acc[ci]);
            }
        }
    }
}

// GSZ = lanes per shell quartet: 64, or 16 (four quartets per wave) for the low angular classes, whose handful of
// components and roots leave a 64-lane wave idle while it waits on its chain of dependent loads.
template <int MAXC, int GSZ>
__global__ __launch_bounds__(64) void eri_rys_kernel(EriArgs A)
{
    extern __shared__ double lds_all[];
    constexpr int QPW = 64 / GSZ;
    const int grp = QPW == 1 ? 0 : threadIdx.x / GSZ, lane = QPW == 1 ? threadIdx.x : threadIdx.x % GSZ;
    const int tl = (int)xcd_block(blockIdx.x, A.xcd) * QPW + grp; // task inside this launch
    if (QPW == 1 && tl >= A.ntask) return;   // (grid rounded up for the XCD map)
    bool live = QPW == 1 || tl < A.ntask;
    const int64_t task = A.t0 + (live ? tl : 0);
    int ib, ik;
    if (A.diag) { ib = (int)task; ik = ib; }
    else get_task(A.tasks, A.prefix, A.nbra, task, ib, ik);
    if (A.swap) { int t_ = ib; ib = ik; ik = t_; }
    const PairRec ab = A.bra[ib], cd = A.ket[ik];
    if (A.qtol > 0.0 && A.scr.q_bra[ib] * A.scr.q_ket[ik] < A.qtol) { if (QPW == 1) return; live = false; }
    if (QPW == 1) { // one quartet per wave: negligible / non-resident quartets leave at once
        if (A.own_table && !quartet_has_resident_tile(A.own_table, ab.ao_i, A.ni, ab.ao_j, A.nj, cd.ao_i, A.nk, cd.ao_j, A.nl, lane)) return;
        if (A.scr.negligible(ib, ik, ab.sh_i, ab.sh_j, cd.sh_i, cd.sh_j)) return;
    } else {
        if (A.own_table)
            live = quartet_has_resident_tile(A.own_table, ab.ao_i, A.ni, ab.ao_j, A.nj, cd.ao_i, A.nk, cd.ao_j, A.nl, lane, GSZ, grp) && live;
        if (A.scr.negligible(ib, ik, ab.sh_i, ab.sh_j, cd.sh_i, cd.sh_j)) live = false;
    }
    const RysLds L{A.PB, A.nroots, A.tsz};
    double *lds = lds_all + (size_t)grp * (L.doubles() + (size_t)A.prim_lds * 8);
    // primitive-pair records {p, P, P-A, K} of the bra and the ket pair: staged once per quartet in LDS (coalesced 64-byte
    // records) so that the R and A phases of every batch read them on-chip instead of paying a global round trip each
    const double *prim_b = A.prim + (size_t)ab.prim_off * 8, *prim_k = A.prim + (size_t)cd.prim_off * 8;
    if (A.prim_lds > 0) {
        double *pl = lds + L.doubles();
        const int nb8 = ab.nprim * 8, nk8 = cd.nprim * 8;
        if (live && ab.nprim + cd.nprim <= A.prim_lds) {
            for (int x = lane; x < nb8; x += GSZ) pl[x] = prim_b[x];
            for (int x = lane; x < nk8; x += GSZ) pl[nb8 + x] = prim_k[x];
            prim_b = pl; prim_k = pl + nb8;
        }
        __syncthreads();
    }
    const int nPQ = live ? ab.nprim * cd.nprim : 0;
    int nPQ_all = nPQ; // uniform trip count over the quartets sharing this wave (the barriers sit in the batch loop)
    if (QPW > 1)
        for (int o = GSZ; o < 64; o <<= 1) nPQ_all = max(nPQ_all, __shfl_xor(nPQ_all, o));
    double *wout = A.work + (size_t)tl * A.ncomp;   // the hand-over buffer
    rys_quartet_body<MAXC, GSZ>(A, prim_b, prim_k, cd.nprim, nPQ, nPQ_all, lane, lds, [&](int c, double v) { wout[c] = v; });
}

typedef double d4_t __attribute__((ext_vector_type(4)));

// One 16x16 tile of C = A B on a single wave with v_mfma_f64_16x16x4_f64 (used by the per-quartet transformation
// kernels, whose matrices are a few tens of rows/columns: one operand load per 16 FMAs instead of two per FMA).
//   A(m,k) = A[m*sam + k*sak] for m < M, B(k,n) = B[k*sbk + n*sbn] for n < N, k < K; out-of-range elements read as 0.
// Result layout: element r of the return value is C[m0 + (lane>>4) + 4r][n0 + (lane&15)].
// Operand loads go out in chunks of WAVE_MFMA_CHUNK k steps before the chunk's MFMAs: the A / B operands of the per-quartet
// transforms come from global memory (per-pair matrices) or LDS, and a load -> wait -> MFMA chain per k step made the kernels
// latency bound (one ~1 us round trip per MFMA: 200 us for an (ff|fd) quartet).
#define WAVE_MFMA_CHUNK 4
__device__ inline d4_t wave_mfma_tile(const double *A, int sam, int sak, int M, const double *B, int sbk, int sbn, int N, int K, int m0,
                                      int n0, int lane)
{
    d4_t acc = {0.0, 0.0, 0.0, 0.0};
    const int m = m0 + (lane & 15), n = n0 + (lane & 15), kq = lane >> 4;
    const bool mv = m < M, nv = n < N;
    const double *pa = A + (size_t)(mv ? m : 0) * sam, *pb = B + (size_t)(nv ? n : 0) * sbn;
    for (int k0 = 0; k0 < K; k0 += 4 * WAVE_MFMA_CHUNK) {
        double av[WAVE_MFMA_CHUNK], bv[WAVE_MFMA_CHUNK];
#pragma unroll
        for (int s_ = 0; s_ < WAVE_MFMA_CHUNK; s_++) {     // the chunk's operand loads go out together: one round trip per 16 k
            const int k = k0 + 4 * s_ + kq;
            const bool kv = k < K;
            av[s_] = (mv && kv) ? pa[(size_t)k * sak] : 0.0;
            bv[s_] = (nv && kv) ? pb[(size_t)k * sbk] : 0.0;
        }
#pragma unroll
        for (int s_ = 0; s_ < WAVE_MFMA_CHUNK; s_++)
            if (k0 + 4 * s_ < K) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s_], bv[s_], acc, 0, 0, 0);
    }
    return acc;
}
// MFMA pays when the zero padding of the 16x16x4 tiles wastes less than ~3/4 of the instruction
__device__ __host__ inline bool mfma_worthwhile(int M, int N, int K)
{
    const int pm = (M + 15) / 16 * 16, pn = (N + 15) / 16 * 16, pk = (K + 3) / 4 * 4;
    return 4 * M * N * K >= pm * pn * pk;
}

// =================================================================================================
// ERI generation, kernel 2: out[ab][cd] = M_ab . E0 . M_cd^T (HRR + cart->sph folded into M), then
// scatter every symmetry image that lands in a canonical resident tile.  One wave per quartet.
// Tile element (i,j,k,l) lives at  off + (((j*4 + l/2) * (bi*bk) + i*bk + k) * 2 + (l&1)).
// =================================================================================================
struct XfArgs {
    const PairRec *bra, *ket;
    const double *Mbuf;
    const int64_t *prefix;
    int nbra;
    int64_t t0, ntask;       // this launch covers tasks [t0, t0+ntask)
    int ne, nf, nsab, nscd, nsb, nsd;
    const double *work;
    int ncomp;
    const int32_t *tile_table;
    const int64_t *tile_off;
    double *tiles;
    int nao;
    int check_owner, ni, nj, nk, nl;
    // density fitting (mi_df_build): dense output instead of the tile scatter.  dense_mode 1: (ij|P) -> dense_out[i][j][P]
    // and [j][i][P] (ld = dense_n auxiliary functions); 2: (P|Q) -> dense_out[P][Q] and [Q][P].  The fitted function of a
    // "pair" (P, unit s) is its first shell.
    double *dense_out;
    int dense_mode, dense_n;
    int tri;                 // triangular rows in block-diagonal tiles (tile geometry)
    const double *q_bra, *q_ket; // with qtol > 0: the same per-task Schwarz rejection as the Rys kernel made
    double qtol;
    unsigned xcd;            // XCD-aware block map (xcd_block)
    const TaskIdx *tasks;    // non-null: (bra, ket) per task, precomputed (get_task)
    int m_lds;               // 1: the two per-pair transformation matrices are staged in LDS with the E0 block (one memory round trip
                             // for all operands; a global load per k step made the products a chain of dependent round trips)
};

// Read-only, wave-uniform operands (work-item records, tile directory, the J-L density rows) go through the
// constant address space so that they are fetched with scalar loads into SGPRs instead of per-lane vector loads.
#define MI_CONST_AS __attribute__((address_space(4)))
template <class T> __device__ inline const MI_CONST_AS T *as_const(const T *p)
{
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    return (const MI_CONST_AS T *)p;
#pragma clang diagnostic pop
}

__device__ inline void put_tile(const XfArgs &A, int i, int j, int k, int l, double v)
{
    int I = i >> 3, J = j >> 3, K = k >> 3, L = l >> 3;
    if (I < J || K < L) return;
    int bij = I * (I + 1) / 2 + J, bkl = K * (K + 1) / 2 + L;
    if (bij < bkl) return;
    // directory look-ups through the constant address space: known not to alias the tile stores, so the compiler may
    // overlap the two dependent loads of one element with those of the next instead of serialising load-load-store chains
    int32_t t = as_const(A.tile_table)[(size_t)bij * (bij + 1) / 2 + bkl];
    if (t < 0) return;
    int bi = min(BLK, A.nao - I * BLK), bk = min(BLK, A.nao - K * BLK);
    double w;
    const int64_t e = tile_elem(A.tri != 0, I == J, K == L, bij == bkl, bi, bk, i & 7, j & 7, k & 7, l & 7, &w);
    if (e >= 0) A.tiles[as_const(A.tile_off)[t] + e] = w * v;
}

// MFMA = true: instantiation with the matrix-core paths for the large angular classes; MFMA = false: lean kernel for
// the small classes that make up most quartets.  GSZ = lanes per quartet (64, or 16 = four quartets per wave, as
// in eri_rys_kernel).  (Four waves sharing a quartet's LDS blocks were measured slower: 0.50 vs 0.46 s for
// ibuprofen/def2-TZVP.)
// element (i,j,k,l) of one symmetry image whose tile base (-1: no resident canonical tile) is already known
__device__ inline void put_tile_at(const XfArgs &A, int64_t base, int i, int j, int k, int l, double v)
{
    if (base < 0) return;
    const int I = i >> 3, J = j >> 3, K = k >> 3, L = l >> 3;
    const int bij = I * (I + 1) / 2 + J, bkl = K * (K + 1) / 2 + L;
    const int bi = min(BLK, A.nao - I * BLK), bk = min(BLK, A.nao - K * BLK);
    double w;
    const int64_t e = tile_elem(A.tri != 0, I == J, K == L, bij == bkl, bi, bk, i & 7, j & 7, k & 7, l & 7, &w);
    if (e >= 0) A.tiles[base + e] = w * v;
}

// FMAXC = 0: the [e0|f0] block comes from the hand-over buffer (A.work) of a preceding eri_rys_kernel launch.
// FMAXC > 0 (GSZ = 64 only): FUSED evaluation -- the Rys phases (rys_quartet_body<FMAXC, 64>, arguments *R) run first in this wave and leave
// the block in LDS: no hand-over buffer (51.8 of the 139.8 GB written by an evaluation of ibuprofen/def2-TZVP), one launch
// and one task look-up per quartet instead of two.
template <bool MFMA, int GSZ, int FMAXC>
__device__ __forceinline__ void xf_body(const XfArgs &A, const EriArgs *R)
{
    extern __shared__ double lds_all[];
    constexpr int QPW = 64 / GSZ;
    __shared__ int64_t tbase_all[QPW][8][16];   // tile base per (symmetry image, 2x2x2x2 sub-block of the quartet's AO ranges)
    const int grp = threadIdx.x / GSZ, lane = threadIdx.x % GSZ;
    const int64_t tl = (int64_t)xcd_block(blockIdx.x, A.xcd) * QPW + grp;
    bool live = tl < A.ntask;
    int ib, ik;
    get_task(A.tasks, A.prefix, A.nbra, A.t0 + (live ? tl : 0), ib, ik);
    const PairRec ab = A.bra[ib], cd = A.ket[ik];
    if (A.qtol > 0.0 && A.q_bra[ib] * A.q_ket[ik] < A.qtol) live = false;
    if (A.check_owner)
        live = quartet_has_resident_tile(A.tile_table, ab.ao_i, A.ni, ab.ao_j, A.nj, cd.ao_i, A.nk, cd.ao_j, A.nl, lane, GSZ, grp) && live;
    if (QPW == 1 && !live) return;
    const double *E0g = FMAXC > 0 ? nullptr : A.work + (size_t)tl * A.ncomp;
    const size_t lds_m = A.m_lds ? (size_t)2 * A.nsab * A.ne + (size_t)2 * A.nscd * A.nf : 0;
    double *E0 = lds_all + (size_t)grp * ((size_t)A.ne * A.nf + (size_t)A.nsab * A.nf + lds_m); // [ne][nf]
    double *X = E0 + A.ne * A.nf;                                                       // [nsab][nf]
    // (M_ab / M_cd^T staged in LDS as well was measured SLOWER -- ibuprofen/def2-TZVP 0.325 -> 0.342 s: this kernel is bound by
    // its scattered tile stores, see DESIGN.md 3.2, and the larger LDS footprint only costs occupancy)
    const double *Mab = A.Mbuf + ab.m_off, *Mcd = A.Mbuf + cd.m_off;
    if (A.m_lds) {   // M and M^T of both pairs, as stored (2 nsab ne and 2 nscd nf doubles)
        double *ML = X + (size_t)A.nsab * A.nf;
        const int na = 2 * A.nsab * A.ne, nc = 2 * A.nscd * A.nf;
        if (live) {
            for (int c = lane; c < na; c += GSZ) ML[c] = Mab[c];
            for (int c = lane; c < nc; c += GSZ) ML[na + c] = Mcd[c];
        }
        Mab = ML; Mcd = ML + na;
    }
    const double *MabT = Mab + A.nsab * A.ne, *McdT = Mcd + A.nscd * A.nf;   // [e][r], [f][c]
    if (FMAXC > 0) {   // (one quartet per wave and live here; the tables lie over the not yet used X block)
        rys_quartet_body<(FMAXC > 0 ? FMAXC : 1), 64>(*R, R->prim + (size_t)ab.prim_off * 8, R->prim + (size_t)cd.prim_off * 8, cd.nprim, ab.nprim * cd.nprim,
                                                       ab.nprim * cd.nprim, lane, X, [&](int c, double v) { E0[c] = v; });
    } else if (live)
        for (int c = lane; c < A.ne * A.nf; c += GSZ) E0[c] = E0g[c];
    // symmetry images: role of (a0,a1,a2,a3) = (ab.i, ab.j, cd.i, cd.j) in (i,j,k,l); bit 0 swaps the bra pair, bit 1 the ket
    // pair, bit 2 exchanges bra and ket.  Which images can land in a canonical tile (I >= J, K >= L) at all is decided once per
    // quartet from the block ranges of the four shells, and so is the tile of every sub-block: the directory look-ups (two
    // dependent global loads) happen 128 times per quartet in parallel instead of once per element and image in sequence.
    const int nsh[4] = {A.nsab / A.nsb, A.nsb, A.nscd / A.nsd, A.nsd};
    const int aos[4] = {ab.ao_i, ab.ao_j, cd.ao_i, cd.ao_j};
    int lo[4], hi[4];
#pragma unroll
    for (int q = 0; q < 4; q++) { lo[q] = aos[q] >> 3; hi[q] = (aos[q] + nsh[q] - 1) >> 3; }
    auto ok = [&](int a, int b, int c, int d) { return hi[a] >= lo[b] && hi[c] >= lo[d]; };
    const unsigned mask = (ok(0, 1, 2, 3) ? 1u : 0u) | (ok(1, 0, 2, 3) ? 2u : 0u) | (ok(0, 1, 3, 2) ? 4u : 0u) | (ok(1, 0, 3, 2) ? 8u : 0u) |
                          (ok(2, 3, 0, 1) ? 16u : 0u) | (ok(3, 2, 0, 1) ? 32u : 0u) | (ok(2, 3, 1, 0) ? 64u : 0u) | (ok(3, 2, 1, 0) ? 128u : 0u);
    int64_t (*tbase)[16] = tbase_all[grp];
    if (live && !A.dense_mode) {
        for (int idx = lane; idx < 128; idx += GSZ) {
            const int img = idx >> 4;
            int64_t base = -1;
            if (mask & (1u << img)) {
                // blocks of the four shells in their own order, then permuted like the indices of this image
                int blk[4];
#pragma unroll
                for (int q = 0; q < 4; q++) blk[q] = lo[q] + ((idx >> q) & 1);
                const bool valid = blk[0] <= hi[0] && blk[1] <= hi[1] && blk[2] <= hi[2] && blk[3] <= hi[3];
                // emit() numbers the exchanged images (l,k,i,j) = 5 and (k,l,j,i) = 6: pair swaps are applied AFTER the exchange there
                const int f = img == 5 ? 6 : (img == 6 ? 5 : img);
                int r0 = (f & 1) ? 1 : 0, r1 = (f & 1) ? 0 : 1, r2 = (f & 2) ? 3 : 2, r3 = (f & 2) ? 2 : 3;
                if (f & 4) { int t_ = r0; r0 = r2; r2 = t_; t_ = r1; r1 = r3; r3 = t_; }
                const int I = blk[r0], J = blk[r1], K = blk[r2], L = blk[r3];
                if (valid && I >= J && K >= L) {
                    const int bij = I * (I + 1) / 2 + J, bkl = K * (K + 1) / 2 + L;
                    if (bij >= bkl) {
                        const int32_t t = A.tile_table[(size_t)bij * (bij + 1) / 2 + bkl];
                        if (t >= 0) base = A.tile_off[t];
                    }
                }
            }
            tbase[img][idx & 15] = base;
        }
    }
    __syncthreads();
    // Result block O[nsab][nscd] goes to LDS first (over E0, which is dead by then), then leaves for the tiles in ADDRESS order.
    double *O = E0;
    auto emit_dense = [&](int r, int c, double s) {   // density fitting: dense (ij|P) / (P|Q) output
        int sa = r / A.nsb, sb = r - sa * A.nsb, sc = c / A.nsd;
        int i = ab.ao_i + sa, j = ab.ao_j + sb, k = cd.ao_i + sc;
        // An element and its mirror image get ONE value from ONE writer, so the output is symmetric to the bit and does not
        // depend on store order: a pair of one shell with itself holds (a,b) and (b,a), and the two-index driver runs both
        // (P|Q) and (Q|P) -- equal in exact arithmetic only.  The image with the larger first index writes both places.
        if (A.dense_mode == 1) {
            if (ab.ao_i == ab.ao_j && i < j) return;
            A.dense_out[((size_t)i * A.nao + j) * A.dense_n + k] = s;
            A.dense_out[((size_t)j * A.nao + i) * A.dense_n + k] = s;
        } else {
            if (i < k) return;
            A.dense_out[(size_t)i * A.dense_n + k] = s;
            A.dense_out[(size_t)k * A.dense_n + i] = s;
        }
    };
    // X = Mab E0, out = X Mcd^T: FP64 MFMA tiles for the large angular classes, per-lane dot products otherwise
    if (MFMA && GSZ == 64 && mfma_worthwhile(A.nsab, A.nf, A.ne)) {
        for (int m0 = 0; m0 < A.nsab; m0 += 16)
            for (int n0 = 0; n0 < A.nf; n0 += 16) {
                d4_t x = wave_mfma_tile(MabT /* M^T [e][r] */, 1, A.nsab, A.nsab, E0, A.nf, 1, A.nf, A.ne, m0, n0, lane);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    int r = m0 + (lane >> 4) + 4 * q, f = n0 + (lane & 15);
                    if (r < A.nsab && f < A.nf) X[r * A.nf + f] = x[q];
                }
            }
    } else if (live) {
        for (int o = lane; o < A.nsab * A.nf; o += GSZ) {
            int r = o / A.nf, f = o - r * A.nf;
            double s = 0.0;
            for (int e = 0; e < A.ne; e++) s += Mab[r * A.ne + e] * E0[e * A.nf + f];
            X[o] = s;
        }
    }
    __syncthreads();
    if (MFMA && GSZ == 64 && mfma_worthwhile(A.nsab, A.nscd, A.nf)) {
        for (int m0 = 0; m0 < A.nsab; m0 += 16)
            for (int n0 = 0; n0 < A.nscd; n0 += 16) {
                d4_t o4 = wave_mfma_tile(X, A.nf, 1, A.nsab, McdT /* M^T [f][c] */, A.nscd, 1, A.nscd, A.nf, m0, n0, lane);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    int r = m0 + (lane >> 4) + 4 * q, c = n0 + (lane & 15);
                    if (r < A.nsab && c < A.nscd) { if (A.dense_mode) emit_dense(r, c, o4[q]); else O[r * A.nscd + c] = o4[q]; }
                }
            }
    } else if (live) {
        for (int o = lane; o < A.nsab * A.nscd; o += GSZ) {
            int r = o / A.nscd, c = o - r * A.nscd;
            double s = 0.0;
            for (int f = 0; f < A.nf; f++) s += X[r * A.nf + f] * McdT[f * A.nscd + c];
            if (A.dense_mode) emit_dense(r, c, s); else O[o] = s;
        }
    }
    if (A.dense_mode) return;
    __syncthreads();
    if (!live) return;
    // Scatter, one symmetry image at a time, in the address order of the tile layout: a tile row is (j, l pair) and inside it
    // the 16-byte chunks run over (i, k), so the lanes enumerate (j | l pair | i | k | l parity) of the image's roles -- one
    // store instruction then covers runs of 2 n_k consecutive doubles per i (48 / 80 / 112 bytes for p / d / f kets) instead of
    // 64 isolated doubles in 64 different rows, and the neighbouring kets (neighbouring tasks, same XCD: xcd_block) complete
    // the lines.  Role tables: image bit 0 swaps the bra pair, bit 1 the ket pair, bit 2 exchanges bra and ket (numbering of
    // `tbase`: 5 = (l,k,i,j), 6 = (k,l,j,i)).
    {
        const int n0_ = nsh[0], n1_ = nsh[1], n2_ = nsh[2], n3_ = nsh[3];
#pragma unroll 1
        for (int img = 0; img < 8; img++) {
            if (!(mask & (1u << img))) continue;
            // shell (0..3 = ab.i, ab.j, cd.i, cd.j) playing the i, j, k, l role of this image
            const int ri = (0x32321010 >> (4 * img)) & 3, rj = (0x23230101 >> (4 * img)) & 3;
            const int rk = (0x11003322 >> (4 * img)) & 3, rl = (0x00112233 >> (4 * img)) & 3;
            auto pick = [](int a, int b, int c_, int d, int q) { return q == 0 ? a : (q == 1 ? b : (q == 2 ? c_ : d)); };
            const int Ni = pick(n0_, n1_, n2_, n3_, ri), Nj = pick(n0_, n1_, n2_, n3_, rj), Nk = pick(n0_, n1_, n2_, n3_, rk),
                      Nl = pick(n0_, n1_, n2_, n3_, rl);
            const int Ai = pick(aos[0], aos[1], aos[2], aos[3], ri), Aj = pick(aos[0], aos[1], aos[2], aos[3], rj),
                      Ak = pick(aos[0], aos[1], aos[2], aos[3], rk), Al = pick(aos[0], aos[1], aos[2], aos[3], rl);
            const int p0 = Al >> 1, npair = ((Al + Nl - 1) >> 1) - p0 + 1;
            const int row = Ni * Nk * 2, tot = Nj * npair * row;
            const float inv_row = 1.0f / (float)row, inv_nk = 1.0f / (float)Nk, inv_np = 1.0f / (float)npair;
            // position of each role's index inside O[(sa nsb + sb) nscd + sc nsd + sd] and inside the sub-block number
            const int st_a = n1_ * A.nscd, st_b = A.nscd, st_c = n3_, st_d = 1;
            const int Si = pick(st_a, st_b, st_c, st_d, ri), Sj = pick(st_a, st_b, st_c, st_d, rj), Sk = pick(st_a, st_b, st_c, st_d, rk),
                      Sl = pick(st_a, st_b, st_c, st_d, rl);
            const int Li = pick(lo[0], lo[1], lo[2], lo[3], ri), Lj = pick(lo[0], lo[1], lo[2], lo[3], rj), Lk = pick(lo[0], lo[1], lo[2], lo[3], rk),
                      Ll = pick(lo[0], lo[1], lo[2], lo[3], rl);
            for (int e = lane; e < tot; e += GSZ) {
                int t = (int)(((float)e + 0.5f) * inv_row);          // (jb, mp) row; exact for these small integers
                const int w = e - t * row;
                const int par = w & 1, h = w >> 1;
                const int ia = (int)(((float)h + 0.5f) * inv_nk), kc = h - ia * Nk;
                const int jb = (int)(((float)t + 0.5f) * inv_np), mp = t - jb * npair;
                const int labs = ((p0 + mp) << 1) + par;
                if (labs < Al || labs >= Al + Nl) continue;
                const double v = O[ia * Si + jb * Sj + kc * Sk + (labs - Al) * Sl];
                const int gi = Ai + ia, gj = Aj + jb, gk = Ak + kc, gl = labs;
                const int sub = (((gi >> 3) - Li) << ri) | (((gj >> 3) - Lj) << rj) | (((gk >> 3) - Lk) << rk) | (((gl >> 3) - Ll) << rl);
                put_tile_at(A, tbase[img][sub], gi, gj, gk, gl, v);
            }
        }
    }
}

template <bool MFMA, int GSZ>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 8))) void eri_transform_scatter(XfArgs A)
{
    xf_body<MFMA, GSZ, 0>(A, nullptr);
}

// Fused evaluation of the mid / high classes: Rys quadrature, HRR + cart->sph products and the scatter of one quartet in ONE wave
// and ONE launch (round 3).  FMAXC = [e0|f0] components per lane kept in registers during the primitive loop.
struct FusedArgs { XfArgs X; EriArgs R; };
template <bool MFMA, int FMAXC>
__global__ __launch_bounds__(64) void eri_fused_kernel(FusedArgs F)
{
    xf_body<MFMA, 64, FMAXC>(F.X, &F.R);
}

// =================================================================================================
// ERI generation for the LOW angular classes: one THREAD per contracted shell quartet, everything in registers, one launch.
//
// The wave-per-quartet pair (eri_rys_kernel + eri_transform_scatter) is latency bound on the classes that make up three
// quarters of all quartets ((ss|ss) ... (dp|ps), (fs|ds)): a handful of components keeps 64 lanes idle and the [e0|f0] block
// makes a round trip through memory between the two kernels.  Here the angular momenta are template parameters, so that the
// primitive loop (Rys roots -> 2-D recurrence -> component products), the horizontal recurrence, the cartesian->spherical
// transforms and the scatter into the resident tiles unroll completely into register code; 64 quartets per wave are in
// flight instead of 1-4.  The Chebyshev coefficients of the Rys roots/weights for this root count (3.5-13 KB) are staged in
// LDS once per workgroup (the per-lane table look-ups then never leave the CU).
// Eligible: NE * NF <= 64 accumulators and <= 3 roots (17 classes up to (dp|ps), (ds|ds), (fs|ds), (fd|ss)).
// =================================================================================================
__host__ __device__ constexpr int c_ncart(int l) { return (l + 1) * (l + 2) / 2; }
__host__ __device__ constexpr int c_cidx(int l, int lx, int ly) { return (l - lx) * (l - lx + 1) / 2 + (l - lx - ly); }
__host__ __device__ constexpr int c_eoff(int la, int deg) { int n = 0; for (int e = la; e < deg; e++) n += c_ncart(e); return n; }
__host__ __device__ constexpr int c_ne(int la, int lb) { return c_eoff(la, la + lb + 1); }
__host__ __device__ constexpr int c_binom(int n, int k) { int r = 1; for (int i = 1; i <= k; i++) r = r * (n - k + i) / i; return r; }

struct TpqArgs {
    const PairRec *bra, *ket;
    const double *prim;
    const int64_t *prefix;
    int nbra;
    int64_t t0, ntask;
    const double *c2s;
    int c2s_off[LMAX + 2];
    RysDev rys;
    XfArgs X;       // tile directory (tile_table, tile_off, tiles, nao) for put_tile
    const double *shell_xyz; // [nbas][3] shell centres (Bohr)
    int check_owner;
    const double *q_bra, *q_ket; // per-task Schwarz rejection (qtol > 0), see EriArgs
    double qtol;
    unsigned xcd;            // XCD-aware block map (xcd_block)
    double omega;            // > 0: erf(omega r12)/r12 integrals (see rys_attenuate)
};

// HRR + cart->sph of one shell pair applied to one index of a register array:
//   in [NE] (E-index, degrees L1 .. L1+L2) -> out [(2L1+1)(2L2+1)];  element (idx, o) lives at idx * SI + o * SO.
template <int L1, int L2, int NO, int SI_IN, int SO_IN, int SI_OUT, int SO_OUT>
__device__ __forceinline__ void tpq_pair_transform(const double *in, double *out, const double AB[3], const MI_CONST_AS double *c1,
                                                   const MI_CONST_AS double *c2)
{
    constexpr int NCA = c_ncart(L1), NCB = c_ncart(L2), NSA = 2 * L1 + 1, NSB = 2 * L2 + 1;
    double pw[3][L2 + 1];
#pragma unroll
    for (int d = 0; d < 3; d++) {
        pw[d][0] = 1.0;
#pragma unroll
        for (int q = 1; q <= L2; q++) pw[d][q] = pw[d][q - 1] * AB[d];
    }
#pragma unroll
    for (int o = 0; o < NO; o++) {
        // horizontal recurrence (closed form): (a b| = sum_{i <= b} C(b,i) AB^(b-i) (a+i 0|
        double g[NCA * NCB];
#pragma unroll
        for (int ax = L1; ax >= 0; ax--)
#pragma unroll
            for (int ay = L1 - ax; ay >= 0; ay--) {
                const int az = L1 - ax - ay, ia = c_cidx(L1, ax, ay);
#pragma unroll
                for (int bx = L2; bx >= 0; bx--)
#pragma unroll
                    for (int by = L2 - bx; by >= 0; by--) {
                        const int bz = L2 - bx - by, ib = c_cidx(L2, bx, by);
                        double v = 0.0;
#pragma unroll
                        for (int ix = 0; ix <= bx; ix++)
#pragma unroll
                            for (int iy = 0; iy <= by; iy++)
#pragma unroll
                                for (int iz = 0; iz <= bz; iz++) {
                                    const int deg = L1 + ix + iy + iz;
                                    const int e = c_eoff(L1, deg) + c_cidx(deg, ax + ix, ay + iy);
                                    const double cf = (double)(c_binom(bx, ix) * c_binom(by, iy) * c_binom(bz, iz));
                                    v = fma(cf * pw[0][bx - ix] * pw[1][by - iy] * pw[2][bz - iz], in[e * SI_IN + o * SO_IN], v);
                                }
                        g[ia * NCB + ib] = v;
                    }
            }
        // cartesian -> spherical on both shells (coefficient tables in constant memory: scalar loads)
        double h[NSA * NCB];
#pragma unroll
        for (int s1 = 0; s1 < NSA; s1++)
#pragma unroll
            for (int b = 0; b < NCB; b++) {
                double v = 0.0;
#pragma unroll
                for (int a = 0; a < NCA; a++) v = fma(c1[a * NSA + s1], g[a * NCB + b], v);
                h[s1 * NCB + b] = v;
            }
#pragma unroll
        for (int s1 = 0; s1 < NSA; s1++)
#pragma unroll
            for (int s2 = 0; s2 < NSB; s2++) {
                double v = 0.0;
#pragma unroll
                for (int b = 0; b < NCB; b++) v = fma(c2[b * NSB + s2], h[s1 * NCB + b], v);
                out[(s1 * NSB + s2) * SI_OUT + o * SO_OUT] = v;
            }
    }
}

#define TPQ_BLOCK 128
static size_t tpq_cheb_bytes(int nr) { return sizeof(double) * (size_t)RYS_NINT_H[nr] * 2 * nr * (RYS_DEG + 1); }
// Chebyshev coefficients of the 2 NR root / weight functions, all intervals, staged in LDS by the workgroup (ends in a barrier)
template <int NR>
__device__ __forceinline__ void tpq_stage_cheb(const RysDev &rys, double *cheb)
{
    const int ntab = rys.nint[NR] * 2 * NR * (RYS_DEG + 1);
    const double *src = rys.cheb + rys.off[NR];
    for (int q = threadIdx.x; q < ntab; q += TPQ_BLOCK) cheb[q] = src[q];
    __syncthreads();
}
template <int LA, int LB, int LC, int LD>
__global__ __launch_bounds__(TPQ_BLOCK) void eri_tpq_kernel(TpqArgs A)
{
    constexpr int NR = (LA + LB + LC + LD) / 2 + 1;
    constexpr int NMAX = LA + LB, MMAX = LC + LD;
    constexpr int NE = c_ne(LA, LB), NF = c_ne(LC, LD);
    constexpr int NSAB = (2 * LA + 1) * (2 * LB + 1), NSCD = (2 * LC + 1) * (2 * LD + 1);
    extern __shared__ double cheb[];
    const int nint = A.rys.nint[NR];
    tpq_stage_cheb<NR>(A.rys, cheb);
    const int64_t tl = (int64_t)xcd_block(blockIdx.x, A.xcd) * TPQ_BLOCK + threadIdx.x;
    if (tl >= A.ntask) return;
    int ib, ik;
    find_task(A.prefix, A.nbra, A.t0 + tl, ib, ik);
    if (A.qtol > 0.0 && A.q_bra[ib] * A.q_ket[ik] < A.qtol) return;
    const PairRec ab = A.bra[ib], cd = A.ket[ik];
    constexpr int ni = 2 * LA + 1, nj = 2 * LB + 1, nk = 2 * LC + 1, nl = 2 * LD + 1;
    // block ranges of the four shells: which index images can land in a canonical tile, and is anything resident here
    const int lo[4] = {ab.ao_i >> 3, ab.ao_j >> 3, cd.ao_i >> 3, cd.ao_j >> 3};
    const int hi[4] = {(ab.ao_i + ni - 1) >> 3, (ab.ao_j + nj - 1) >> 3, (cd.ao_i + nk - 1) >> 3, (cd.ao_j + nl - 1) >> 3};
    if (A.check_owner && !quartet_has_resident_tile_thread(A.X.tile_table, ab.ao_i, ni, ab.ao_j, nj, cd.ao_i, nk, cd.ao_j, nl)) return;

    double acc[NE * NF];
#pragma unroll
    for (int q = 0; q < NE * NF; q++) acc[q] = 0.0;
    for (int ip = 0; ip < ab.nprim; ip++) {
        const double *b = A.prim + (size_t)(ab.prim_off + ip) * 8;
        const double p = b[0], Px = b[1], Py = b[2], Pz = b[3], Kab = b[7];
        const double PA[3] = {b[4], b[5], b[6]};
        for (int jp = 0; jp < cd.nprim; jp++) {
            const double *kk = A.prim + (size_t)(cd.prim_off + jp) * 8;
            const double q = kk[0];
            const double PQ[3] = {Px - kk[1], Py - kk[2], Pz - kk[3]};
            const double QC[3] = {kk[4], kk[5], kk[6]};
            const double pq1 = 1.0 / (p + q);
            double x = p * q * pq1 * (PQ[0] * PQ[0] + PQ[1] * PQ[1] + PQ[2] * PQ[2]);
            double pref = Kab * kk[7] * 34.986836655249725 /* 2 pi^2.5 */ * pq1 * sqrt(p + q) / (p * q);
            double th = 1.0;   // long-range store: argument x theta, roots u theta (below), prefactor sqrt(theta) (rys_attenuate)
            if (A.omega > 0.0) {
                const double w2 = A.omega * A.omega;
                th = w2 / (w2 + p * q * pq1);
                x *= th;
                pref *= sqrt(th);
            }
            // Rys roots u_r and weights w_r: Chebyshev interpolation from the LDS copy, asymptotic form beyond the table
            double u[NR], w[NR];
            if (x < nint * RYS_H) {
                int iv = (int)(x * (1.0 / RYS_H));
                if (iv >= nint) iv = nint - 1;
                const double sx = (x - (iv * RYS_H + 0.5 * RYS_H)) * (2.0 / RYS_H), s2 = 2.0 * sx;
                const double *cb = cheb + (size_t)iv * 2 * NR * (RYS_DEG + 1);
#pragma unroll
                for (int f = 0; f < 2 * NR; f++) {
                    const double *cc = cb + f * (RYS_DEG + 1);
                    double b1 = 0.0, b2 = 0.0;
#pragma unroll
                    for (int kq = RYS_DEG; kq >= 1; kq--) {
                        double tq = s2 * b1 - b2 + cc[kq];
                        b2 = b1;
                        b1 = tq;
                    }
                    const double val = sx * b1 - b2 + cc[0];
                    if (f < NR) u[f] = val; else w[f - NR] = val;
                }
            } else {
                const double rx = 1.0 / x, rsx = rsqrt(x);
#pragma unroll
                for (int f = 0; f < NR; f++) { u[f] = A.rys.herm_r[NR * RYS_NMAX + f] * rx; w[f] = A.rys.herm_w[NR * RYS_NMAX + f] * rsx; }
            }
            if (A.omega > 0.0) {
#pragma unroll
                for (int f = 0; f < NR; f++) u[f] *= th;
            }
#pragma unroll
            for (int r = 0; r < NR; r++) {
                const double ur = u[r];
                const double b00 = 0.5 * ur * pq1, b10 = 0.5 / p * (1.0 - ur * q * pq1), b01 = 0.5 / q * (1.0 - ur * p * pq1);
                double T[3][NMAX + 1][MMAX + 1];
#pragma unroll
                for (int d = 0; d < 3; d++) {
                    const double c00 = PA[d] - ur * q * pq1 * PQ[d], c01 = QC[d] + ur * p * pq1 * PQ[d];
                    T[d][0][0] = d == 2 ? w[r] * pref : 1.0;
#pragma unroll
                    for (int n = 0; n < NMAX; n++) T[d][n + 1][0] = c00 * T[d][n][0] + (n > 0 ? n * b10 * T[d][n - 1][0] : 0.0);
#pragma unroll
                    for (int m = 0; m < MMAX; m++)
#pragma unroll
                        for (int n = 0; n <= NMAX; n++) {
                            double v = c01 * T[d][n][m];
                            if (m > 0) v = fma(m * b01, T[d][n][m - 1], v);
                            if (n > 0) v = fma(n * b00, T[d][n - 1][m], v);
                            T[d][n][m + 1] = v;
                        }
                }
                // component products: e = (ex,ey,ez) of degree LA..LA+LB, f of degree LC..LC+LD (orders as build_comp_table)
#pragma unroll
                for (int de = LA; de <= LA + LB; de++)
#pragma unroll
                    for (int ex = de; ex >= 0; ex--)
#pragma unroll
                        for (int ey = de - ex; ey >= 0; ey--) {
                            const int ez = de - ex - ey, ie = c_eoff(LA, de) + c_cidx(de, ex, ey);
#pragma unroll
                            for (int df = LC; df <= LC + LD; df++)
#pragma unroll
                                for (int fx = df; fx >= 0; fx--)
#pragma unroll
                                    for (int fy = df - fx; fy >= 0; fy--) {
                                        const int fz = df - fx - fy, jf = c_eoff(LC, df) + c_cidx(df, fx, fy);
                                        acc[ie * NF + jf] = fma(T[0][ex][fx] * T[1][ey][fy], T[2][ez][fz], acc[ie * NF + jf]);
                                    }
                        }
            }
        }
    }
    // HRR + cart->sph: bra index first ([NE][NF] -> [NSAB][NF]), then the ket index ([NSAB][NF] -> [NSAB][NSCD])
    const MI_CONST_AS double *c2s = as_const(A.c2s);
    // AB = A - B of each pair (first minus second shell of the record) from the shell centres
    double ABv[3], CDv[3];
#pragma unroll
    for (int d = 0; d < 3; d++) {
        ABv[d] = A.shell_xyz[3 * ab.sh_i + d] - A.shell_xyz[3 * ab.sh_j + d];
        CDv[d] = A.shell_xyz[3 * cd.sh_i + d] - A.shell_xyz[3 * cd.sh_j + d];
    }
    double X1[NSAB * NF];
    tpq_pair_transform<LA, LB, NF, NF, 1, NF, 1>(acc, X1, ABv, c2s + A.c2s_off[LA], c2s + A.c2s_off[LB]);
    double out[NSAB * NSCD];
    tpq_pair_transform<LC, LD, NSAB, 1, NF, 1, NSCD>(X1, out, CDv, c2s + A.c2s_off[LC], c2s + A.c2s_off[LD]);
    // scatter every symmetry image that lands in a canonical resident tile.  The directory look-up (two dependent global
    // loads) is done once per change of tile, not per element: the elements of an image touch at most 16 tiles, usually one.
    auto ok = [&](int a, int b, int c, int d) { return hi[a] >= lo[b] && hi[c] >= lo[d]; };
    const unsigned mask = (ok(0, 1, 2, 3) ? 1u : 0u) | (ok(1, 0, 2, 3) ? 2u : 0u) | (ok(0, 1, 3, 2) ? 4u : 0u) | (ok(1, 0, 3, 2) ? 8u : 0u) |
                          (ok(2, 3, 0, 1) ? 16u : 0u) | (ok(3, 2, 0, 1) ? 32u : 0u) | (ok(2, 3, 1, 0) ? 64u : 0u) | (ok(3, 2, 1, 0) ? 128u : 0u);
    const MI_CONST_AS int32_t *ttab = as_const(A.X.tile_table);
    const MI_CONST_AS int64_t *toff = as_const(A.X.tile_off);
    const int nao = A.X.nao;
#pragma unroll
    for (int img = 0; img < 8; img++) {
        // images 5 and 6 of this construction are (k,l,j,i) and (l,k,i,j): bits 6 and 5 of the block-range mask
        const int mbit = img == 5 ? 6 : (img == 6 ? 5 : img);
        if (!(mask & (1u << mbit))) continue;
        size_t slot_c = ~(size_t)0;
        int64_t base_c = -1;
#pragma unroll
        for (int sa = 0; sa < ni; sa++)
#pragma unroll
            for (int sb = 0; sb < nj; sb++)
#pragma unroll
                for (int sc = 0; sc < nk; sc++)
#pragma unroll
                    for (int sd = 0; sd < nl; sd++) {
                        const int a0 = ab.ao_i + sa, a1 = ab.ao_j + sb, a2 = cd.ao_i + sc, a3 = cd.ao_j + sd;
                        // image `img`: bit 0 swaps the bra pair, bit 1 the ket pair, bit 2 exchanges bra and ket
                        int i = (img & 1) ? a1 : a0, j = (img & 1) ? a0 : a1, k = (img & 2) ? a3 : a2, l = (img & 2) ? a2 : a3;
                        if (img & 4) { int t_ = i; i = k; k = t_; t_ = j; j = l; l = t_; }
                        const int I = i >> 3, J = j >> 3, K = k >> 3, L = l >> 3;
                        if (I < J || K < L) continue;
                        const int bij = I * (I + 1) / 2 + J, bkl = K * (K + 1) / 2 + L;
                        if (bij < bkl) continue;
                        const size_t slot = (size_t)bij * (bij + 1) / 2 + bkl;
                        if (slot != slot_c) {
                            slot_c = slot;
                            const int32_t t = ttab[slot];
                            base_c = t >= 0 ? toff[t] : -1;
                        }
                        if (base_c < 0) continue;
                        const int bi = min(BLK, nao - I * BLK), bk = min(BLK, nao - K * BLK);
                        double w;
                        const int64_t e = tile_elem(A.X.tri != 0, I == J, K == L, bij == bkl, bi, bk, i & 7, j & 7, k & 7, l & 7, &w);
                        if (e >= 0) A.X.tiles[base_c + e] = w * out[(sa * nj + sb) * NSCD + sc * nl + sd];
                    }
    }
}

// Schwarz: q[b] = sqrt(max_ab |(ab|ab)|) from the diagonal-task E0 blocks.
struct SchwarzArgs {
    const PairRec *bra;
    const double *Mbuf;
    const double *work;
    int ne, nsab, ncomp;
    double *q;
};
__global__ __launch_bounds__(64) void schwarz_diag_kernel(SchwarzArgs A)
{
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const PairRec ab = A.bra[blockIdx.x];
    const double *E0g = A.work + (size_t)blockIdx.x * A.ncomp;
    for (int c = lane; c < A.ne * A.ne; c += 64) lds[c] = E0g[c];
    __syncthreads();
    const double *M = A.Mbuf + ab.m_off;
    double mx = 0.0;
    for (int r = lane; r < A.nsab; r += 64) {
        double s = 0.0;
        for (int e = 0; e < A.ne; e++) {
            double t = 0.0;
            for (int f = 0; f < A.ne; f++) t += lds[e * A.ne + f] * M[r * A.ne + f];
            s += M[r * A.ne + e] * t;
        }
        mx = fmax(mx, fabs(s));
    }
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
    if (lane == 0) A.q[blockIdx.x] = sqrt(mx);
}

// =================================================================================================
// Host side of ERI preparation
// =================================================================================================
static void build_comp_table(int la, int lb, int lc, int ld, std::vector<uint32_t> &comp)
{
    int M1 = lc + ld + 1;
    comp.clear();
    for (int e = la; e <= la + lb; e++)
        for (int ex = e; ex >= 0; ex--)
            for (int ey = e - ex; ey >= 0; ey--) {
                int ez = e - ex - ey;
                for (int f = lc; f <= lc + ld; f++)
                    for (int fx = f; fx >= 0; fx--)
                        for (int fy = f - fx; fy >= 0; fy--) {
                            int fz = f - fx - fy;
                            uint32_t ix = ex * M1 + fx, iy = ey * M1 + fy, iz = ez * M1 + fz;
                            comp.push_back(ix | (iy << 10) | (iz << 20));
                        }
            }
}

// M[(sa,sb)][e] = sum_{a,b cart} c2s_a[a][sa] c2s_b[b][sb] prod_d C(b_d,i_d) AB_d^(b_d-i_d), e = a + i
static void build_M(int la, int lb, const double AB[3], const std::vector<double> &ca, const std::vector<double> &cb,
                    double *M /* [nsa*nsb][ne] */)
{
    int nsa = 2 * la + 1, nsb = 2 * lb + 1, ne = ne_of(la, lb);
    std::fill(M, M + (size_t)nsa * nsb * ne, 0.0);
    // e-offsets by degree
    int eoff[2 * LMAX + 2];
    eoff[la] = 0;
    for (int e = la; e < la + lb + 1; e++) eoff[e + 1] = eoff[e] + ncart(e);
    double pw[3][LMAX + 1];
    for (int d = 0; d < 3; d++) { pw[d][0] = 1.0; for (int k = 1; k <= LMAX; k++) pw[d][k] = pw[d][k - 1] * AB[d]; }
    int ia = 0;
    for (int ax = la; ax >= 0; ax--)
        for (int ay = la - ax; ay >= 0; ay--, ia++) {
            int az = la - ax - ay;
            int ibx = 0;
            for (int bx = lb; bx >= 0; bx--)
                for (int by = lb - bx; by >= 0; by--, ibx++) {
                    int bz = lb - bx - by;
                    for (int ix = 0; ix <= bx; ix++)
                        for (int iy = 0; iy <= by; iy++)
                            for (int iz = 0; iz <= bz; iz++) {
                                double coef = binom(bx, ix) * binom(by, iy) * binom(bz, iz) * pw[0][bx - ix] * pw[1][by - iy] * pw[2][bz - iz];
                                int deg = la + ix + iy + iz;
                                int e = eoff[deg] + cart_index(deg, ax + ix, ay + iy);
                                for (int sa = 0; sa < nsa; sa++) {
                                    double c1 = ca[(size_t)ia * nsa + sa];
                                    if (c1 == 0.0) continue;
                                    for (int sb = 0; sb < nsb; sb++) {
                                        double c2 = cb[(size_t)ibx * nsb + sb];
                                        if (c2 != 0.0) M[(size_t)(sa * nsb + sb) * ne + e] += c1 * c2 * coef;
                                    }
                                }
                            }
                }
        }
}

// coarse[g] = largest bra index ib with prefix[ib] <= g*1024, for g = 0 .. ntask/1024 + 1 (appended to `prefix`)
static void append_coarse_index(std::vector<int64_t> &prefix)
{
    const int nbra = (int)prefix.size() - 1;
    const int64_t ntask = prefix.back();
    const int64_t ng = (ntask >> 10) + 2;
    prefix.reserve(prefix.size() + (size_t)ng);
    int ib = 0;
    for (int64_t g = 0; g < ng; g++) {
        const int64_t t = g << 10;
        while (ib < nbra && prefix[ib + 1] <= t) ib++;
        prefix.push_back(ib);
    }
}

// Task list of a (bra class, ket class) pair: bra b visits the leading kets of the (bound-ordered, see mi_eri_prepare step 3)
// ket list whose bound cq can pass the Schwarz test with the bra's own q; inside one class only kets up to the bra itself
// (canonical quartets).  `prefix` = cumulative counts + the coarse search index; returns the number of tasks.  Kets inside a
// surviving cluster whose own q fails the test are rejected per task by the kernels (qtol).
static int64_t class_prefix(const PairClass &B, const PairClass &Kc, bool same, double tol, std::vector<int64_t> &prefix)
{
    prefix.assign(B.recs.size() + 1, 0);
    for (size_t b = 0; b < B.recs.size(); b++) {
        const double thr = tol / B.q[b];
        size_t lo = 0, hi = Kc.cq.size();
        while (lo < hi) { size_t mid = (lo + hi) / 2; if (Kc.cq[mid] >= thr) lo = mid + 1; else hi = mid; }
        int64_t cnt = (int64_t)lo;
        if (same) cnt = std::min<int64_t>(cnt, (int64_t)b + 1);
        prefix[b + 1] = prefix[b] + cnt;
    }
    const int64_t ntask = prefix.back();
    append_coarse_index(prefix);
    return ntask;
}

// Classes that run four quartets per wave (measured per class on ibuprofen/def2-TZVP: with more roots or components
// the 16-lane groups need more primitive batches / passes than they win by overlapping four latency chains).
static bool eri_small_class(const EriArgs &E) { return E.nroots <= 2 && E.ncomp <= 18; }

// LDS bytes of one quartet in eri_rys_kernel: its Rys block and the staged primitive records
static size_t eri_rys_lds_bytes(const EriArgs &E) { return sizeof(double) * (RysLds{E.PB, E.nroots, E.tsz}.doubles() + (size_t)E.prim_lds * 8); }

static int launch_eri(mi_ctx *c, EriArgs &E, int nblocks, hipStream_t st)
{
    // E.ntask tasks; the low angular classes run four quartets per wave (16 lanes each) unless their contraction depth
    // makes the four quartets of a wave too unequal: cost model in primitive batches per four quartets
    if (E.ntask != nblocks) return fail("launch_eri: ntask/grid mismatch");
    if (nblocks < 2048) E.xcd = 0;   // too small for the chunked map to matter
    int perlane = (E.ncomp + 63) / 64;
    if (eri_small_class(E) && !E.diag && E.h_shared_np > 0.0) {
        const int pb16 = std::max(1, 16 / (3 * E.nroots)), pb64 = std::max(1, 64 / (3 * E.nroots));
        const double cost16 = std::ceil(E.h_shared_np * E.h_vary_max4 / pb16) + 1.5;
        const double cost64 = 4.0 * (std::ceil(E.h_shared_np * E.h_vary_mean / pb64) + 1.5);
        if (cost16 < cost64) {
            EriArgs G = E;
            G.PB = pb16;
            const size_t shm = 4 * eri_rys_lds_bytes(G);
            hipLaunchKernelGGL((eri_rys_kernel<2, 16>), dim3(eri_grid((nblocks + 3) / 4, G.xcd)), dim3(64), shm, st, G);
            HIPCHK(hipGetLastError());
            return 0;
        }
    }
    // Round 3: four quartets per wave also for the MID classes when the contraction is shallow (uncontracted d / f shells: one
    // primitive quartet keeps 2 n of 64 lanes busy in the root phase and 3 n in the recurrence phase of a one-quartet wave).
    if (c->opt_rys_qpw_maxcomp > 0 && !E.diag && E.nroots <= 5 && E.ncomp > 18 && E.ncomp <= c->opt_rys_qpw_maxcomp && E.h_shared_np > 0.0 &&
        E.h_shared_np * E.h_vary_max4 <= c->opt_rys_qpw_maxprim) {
        EriArgs G = E;
        G.PB = std::max(1, 16 / (3 * E.nroots));
        const size_t shm = 4 * eri_rys_lds_bytes(G);
        const dim3 grid(eri_grid((nblocks + 3) / 4, G.xcd));
        const int per16 = (E.ncomp + 15) / 16;
        if (shm <= 64 * 1024) {
            if (per16 <= 4) hipLaunchKernelGGL((eri_rys_kernel<4, 16>), grid, dim3(64), shm, st, G);
            else if (per16 <= 8) hipLaunchKernelGGL((eri_rys_kernel<8, 16>), grid, dim3(64), shm, st, G);
            else hipLaunchKernelGGL((eri_rys_kernel<16, 16>), grid, dim3(64), shm, st, G);
            HIPCHK(hipGetLastError());
            return 0;
        }
    }
    const size_t shm = eri_rys_lds_bytes(E);
    if (perlane <= 1) hipLaunchKernelGGL((eri_rys_kernel<1, 64>), dim3(eri_grid(nblocks, E.xcd)), dim3(64), shm, st, E);
    else if (perlane <= 2 && c->opt_rys_fine) hipLaunchKernelGGL((eri_rys_kernel<2, 64>), dim3(eri_grid(nblocks, E.xcd)), dim3(64), shm, st, E);
    else if (perlane <= 4) hipLaunchKernelGGL((eri_rys_kernel<4, 64>), dim3(eri_grid(nblocks, E.xcd)), dim3(64), shm, st, E);
    else if (perlane <= 8 && c->opt_rys_fine) hipLaunchKernelGGL((eri_rys_kernel<8, 64>), dim3(eri_grid(nblocks, E.xcd)), dim3(64), shm, st, E);
    else if (perlane <= 16) hipLaunchKernelGGL((eri_rys_kernel<16, 64>), dim3(eri_grid(nblocks, E.xcd)), dim3(64), shm, st, E);
    else hipLaunchKernelGGL((eri_rys_kernel<32, 64>), dim3(eri_grid(nblocks, E.xcd)), dim3(64), shm, st, E);
    HIPCHK(hipGetLastError());
    return 0;
}

static void setup_eri_dims(EriArgs &E, int la, int lb, int lc, int ld)
{
    E.la = la; E.lb = lb; E.lc = lc; E.ld = ld;
    E.nmax = la + lb; E.mmax = lc + ld;
    E.nroots = (la + lb + lc + ld) / 2 + 1;
    E.tsz = ((E.nmax + 1) * (E.mmax + 1)) | 1; // table stride in LDS, odd so that the per-(slot,direction) tables start in different banks
    E.ncomp = ne_of(la, lb) * ne_of(lc, ld);
    int pb = 64 / (3 * E.nroots);
    E.PB = std::max(1, pb);
}

// Launch the thread-per-quartet kernel of an eligible class: returns 1 if launched, 0 if the class is not covered, -1 on error.
template <int LA, int LB, int LC, int LD>
static int launch_eri_tpq_t(const TpqArgs &Q, hipStream_t st)
{
    const size_t shm = tpq_cheb_bytes((LA + LB + LC + LD) / 2 + 1);
    const int64_t MAXB = (int64_t)1 << 24;
    for (int64_t t0 = 0; t0 < Q.ntask; t0 += MAXB * TPQ_BLOCK) {   // grid.x stays well below 2^31 (also after the XCD-map rounding)
        TpqArgs P = Q;
        P.t0 = Q.t0 + t0;
        P.ntask = std::min<int64_t>(Q.ntask - t0, MAXB * TPQ_BLOCK);
        const int64_t nblk = (P.ntask + TPQ_BLOCK - 1) / TPQ_BLOCK;
        if (nblk < 1024) P.xcd = 0;
        hipLaunchKernelGGL((eri_tpq_kernel<LA, LB, LC, LD>), dim3(eri_grid(nblk, P.xcd)), dim3(TPQ_BLOCK), shm, st, P);
    }
    if (hipGetLastError() != hipSuccess) return fail("eri_tpq_kernel launch failed");
    return 1;
}

// returns 1 if the class has a thread-per-quartet kernel (and it was launched), 0 if not, -1 on error.  dry: only answers the question
static int launch_eri_tpq(int la, int lb, int lc, int ld, const TpqArgs &Q, hipStream_t st, bool dry = false)
{
    if (la > 3 || lb > 3 || lc > 3 || ld > 3) return 0;
    const int key = ((la * 4 + lb) * 4 + lc) * 4 + ld;
#define TPQ_CASE(a, b, c_, d) case (((a) * 4 + (b)) * 4 + (c_)) * 4 + (d): return dry ? 1 : launch_eri_tpq_t<a, b, c_, d>(Q, st)
    switch (key) {
        TPQ_CASE(0, 0, 0, 0); TPQ_CASE(1, 0, 0, 0); TPQ_CASE(1, 0, 1, 0); TPQ_CASE(1, 1, 0, 0); TPQ_CASE(1, 1, 1, 0);
        TPQ_CASE(2, 0, 0, 0); TPQ_CASE(2, 0, 1, 0); TPQ_CASE(2, 0, 1, 1); TPQ_CASE(2, 0, 2, 0); TPQ_CASE(2, 1, 0, 0);
        TPQ_CASE(2, 1, 1, 0); TPQ_CASE(2, 2, 0, 0); TPQ_CASE(3, 0, 0, 0); TPQ_CASE(3, 0, 1, 0); TPQ_CASE(3, 0, 2, 0);
        TPQ_CASE(3, 1, 0, 0); TPQ_CASE(3, 2, 0, 0);
        TPQ_CASE(2, 1, 2, 0); TPQ_CASE(2, 2, 1, 0); TPQ_CASE(3, 3, 0, 0);   // 96 / 93 / 74 accumulators: one wave per SIMD, still ahead
        TPQ_CASE(3, 1, 1, 0); TPQ_CASE(3, 0, 1, 1); TPQ_CASE(3, 0, 3, 0);   // round 3 candidates: 75 / 90 / 100 accumulators
    default: return 0;
    }
#undef TPQ_CASE
}
static bool tpq_has_class(int la, int lb, int lc, int ld)
{
    TpqArgs none{};
    return launch_eri_tpq(la, lb, lc, ld, none, nullptr, true) == 1;
}

// Sharding plan of the resident tile store: enumerate the (J,K,L) runs that survive the block-pair
// Schwarz test, then deal them to ranks longest-processing-time first (largest run to the least loaded rank) by the bytes a
// J/K build streams for them.  Pure host code and a pure function of its arguments, so every rank derives the same plan.
struct RunPlan { int J, K, L, count, owner; int64_t bytes; };

// doubles a tile occupies in the store: its chunks, rounded up to 256 bytes so that rows of following tiles stay sector-aligned
static inline int64_t tile_doubles_padded(bool dij, bool dkl, int bi, int bk) { return ((int64_t)tile_chunks(dij, dkl, bi, bk) * 2 + 31) / 32 * 32; }

static void plan_runs(int nao, const std::vector<double> &Qblk, double qmax, double tol, int nranks, bool tri, std::vector<RunPlan> &plan)
{
    const int nblk = (nao + BLK - 1) / BLK, nbp = nblk * (nblk + 1) / 2;
    auto bsize = [&](int B) { return std::min(BLK, nao - B * BLK); };
    plan.clear();
    // (13.6 M candidate tiles for ibuprofen/def2-TZVP: the ket block pairs are scanned by the host threads, their run lists
    // joined in kl order -- the plan does not depend on the number of threads)
    std::vector<std::vector<RunPlan>> per(nbp);
#pragma omp parallel for schedule(dynamic, 8) num_threads(host_threads())
    for (int kl = 0; kl < nbp; kl++) {
        if (!(Qblk[kl] * qmax >= tol)) continue;
        int K = (int)((std::sqrt(8.0 * kl + 1.0) - 1.0) / 2.0);
        while ((K + 1) * (K + 2) / 2 <= kl) K++;
        while (K * (K + 1) / 2 > kl) K--;
        const int L = kl - K * (K + 1) / 2;
        const int bk = bsize(K);
        for (int J = 0; J < nblk; J++) {
            RunPlan r{J, K, L, 0, 0, 0};
            for (int I = J; I < nblk; I++) {
                int ij = I * (I + 1) / 2 + J;
                if (ij < kl || Qblk[ij] * Qblk[kl] < tol) continue;
                r.count++;
                r.bytes += tile_doubles_padded(tri && I == J, tri && K == L, bsize(I), bk) * 8;
            }
            if (r.count) per[kl].push_back(r);
        }
    }
    size_t nrun = 0;
    for (const auto &v : per) nrun += v.size();
    plan.reserve(nrun);
    for (const auto &v : per) plan.insert(plan.end(), v.begin(), v.end());
    if (nranks <= 1) return;
    std::vector<int> ord(plan.size());
    std::iota(ord.begin(), ord.end(), 0);
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return plan[a].bytes > plan[b].bytes; });
    // least-loaded rank: binary heap of (load, rank); ties go to the lower rank so the plan is reproducible
    std::vector<std::pair<int64_t, int>> heap(nranks);
    for (int r = 0; r < nranks; r++) heap[r] = {0, r};
    auto cmp = [](const std::pair<int64_t, int> &a, const std::pair<int64_t, int> &b) { return a > b; }; // min-heap
    std::make_heap(heap.begin(), heap.end(), cmp);
    for (int o : ord) {
        std::pop_heap(heap.begin(), heap.end(), cmp);
        plan[o].owner = heap.back().second;
        heap.back().first += plan[o].bytes;
        std::push_heap(heap.begin(), heap.end(), cmp);
    }
}

// Host-only view of the plan (no GPU, no context): bytes streamed per rank for a given block-pair Schwarz table
// qblk[nbp] (nbp = nblk(nblk+1)/2, nblk = ceil(nao/8), pair index I(I+1)/2+J).  Used by the CPU tests of the balance.
extern "C" int mi_plan_shards(int nao, const double *qblk, double tol, int nranks, int64_t *bytes_per_rank, int64_t *runs_per_rank)
{
    if (nao <= 0 || !qblk || nranks < 1 || !bytes_per_rank) return fail("mi_plan_shards: bad argument");
    const int nblk = (nao + BLK - 1) / BLK, nbp = nblk * (nblk + 1) / 2;
    std::vector<double> Q(qblk, qblk + nbp);
    double qmax = 0.0;
    for (double v : Q) qmax = std::max(qmax, v);
    std::vector<RunPlan> plan;
    plan_runs(nao, Q, qmax, tol, nranks, true, plan);
    for (int r = 0; r < nranks; r++) { bytes_per_rank[r] = 0; if (runs_per_rank) runs_per_rank[r] = 0; }
    for (const RunPlan &p : plan) { bytes_per_rank[p.owner] += p.bytes; if (runs_per_rank) runs_per_rank[p.owner]++; }
    return 0;
}

static std::vector<std::vector<double>> c2s_tables()
{
    std::vector<std::vector<double>> c2s(LMAX + 1);
    for (int l = 0; l <= LMAX; l++) c2s_generic(l, c2s[l]);
    return c2s;
}

// ---- Primitive-pair records of a shell pair (I, J): 8 doubles {p, Px, Py, Pz, PAx, PAy, PAz, K} per primitive pair, the
// primitives of I outermost.  Primitive pairs with mu r^2 > 80 are dropped.  Every driver (mi_eri_prepare, mi_df_build, the
// variant records of the two gradients) counts and writes through these two functions: the record order defines
// PairRec::prim_off, so the count and the writer must agree to the bit.
static int count_prim_pairs(const ShellH &I, const ShellH &J)
{
    double r2 = 0.0;
    for (int d = 0; d < 3; d++) r2 += (I.r[d] - J.r[d]) * (I.r[d] - J.r[d]);
    int np = 0;
    for (int ip = 0; ip < I.nprim; ip++)
        for (int jp = 0; jp < J.nprim; jp++)
            if (I.exps[ip] * J.exps[jp] / (I.exps[ip] + J.exps[jp]) * r2 <= 80.0) np++;
    return np;
}
// Writes the records to `dst` (room for I.nprim * J.nprim of them) and returns their number.  times_2a: the coefficient of
// I's primitive carries 2 alpha (the l+1 variant of a differentiated shell, see the gradient section).
static int write_prim_pairs(const ShellH &I, const ShellH &J, bool times_2a, double *dst)
{
    double AB[3] = {I.r[0] - J.r[0], I.r[1] - J.r[1], I.r[2] - J.r[2]};
    double r2 = AB[0] * AB[0] + AB[1] * AB[1] + AB[2] * AB[2];
    int np = 0;
    for (int ip = 0; ip < I.nprim; ip++)
        for (int jp = 0; jp < J.nprim; jp++) {
            double a = I.exps[ip], b = J.exps[jp], p = a + b, mu = a * b / p;
            if (mu * r2 > 80.0) continue; // exp(-80) = 1.8e-35: below double resolution of any sum
            double K = I.coef[ip] * J.coef[jp] * std::exp(-mu * r2) * (times_2a ? 2.0 * a : 1.0);
            double Pc[3];
            for (int d = 0; d < 3; d++) Pc[d] = (a * I.r[d] + b * J.r[d]) / p;
            double rec[8] = {p, Pc[0], Pc[1], Pc[2], Pc[0] - I.r[0], Pc[1] - I.r[1], Pc[2] - I.r[2], K};
            memcpy(dst, rec, sizeof rec);
            dst += 8;
            np++;
        }
    return np;
}
static int append_prim_pairs(const ShellH &I, const ShellH &J, std::vector<double> &prim)
{
    const size_t at = prim.size();
    prim.resize(at + (size_t)8 * I.nprim * J.nprim);
    const int np = write_prim_pairs(I, J, false, prim.data() + at);
    prim.resize(at + (size_t)8 * np);
    return np;
}
// The auxiliary "pair" (P, unit s function) of density fitting: p = alpha, centre P = A, P - A = 0, K = c_P * c_unit
static void write_aux_prims(const ShellH &S, const ShellH &U, double *dst)
{
    for (int ip = 0; ip < S.nprim; ip++) {
        double rec[8] = {S.exps[ip], S.r[0], S.r[1], S.r[2], 0.0, 0.0, 0.0, S.coef[ip] * U.coef[0]};
        memcpy(dst + (size_t)8 * ip, rec, sizeof rec);
    }
}
// M [nsab][ne] (build_M) followed by its transpose [ne][nsab]: the MFMA transform reads both operands with the lane index on
// the contiguous dimension
static void build_M_and_transpose(int la, int lb, const double AB[3], const std::vector<double> &ca, const std::vector<double> &cb, double *M)
{
    build_M(la, lb, AB, ca, cb, M);
    const int nsab = (2 * la + 1) * (2 * lb + 1), ne = ne_of(la, lb);
    double *Mt = M + (size_t)nsab * ne;
    for (int r = 0; r < nsab; r++)
        for (int e = 0; e < ne; e++) Mt[(size_t)e * nsab + r] = M[(size_t)r * ne + e];
}

// ---- Set-up of one pass over a (bra class, ket class) pair, shared by the four integral drivers
// dense task list: every bra meets all `nket` kets (density fitting)
static int64_t dense_prefix(int nbra, int nket, std::vector<int64_t> &prefix)
{
    prefix.resize((size_t)nbra + 1);
    for (int b = 0; b <= nbra; b++) prefix[b] = (int64_t)b * nket;
    const int64_t ntask = prefix.back();
    append_coarse_index(prefix);
    return ntask;
}
// the copy is asynchronous: `prefix` must live until the stream is synchronised (upload_comp_table below does)
static int prefix_to_device(const std::vector<int64_t> &prefix, DevBuf<int64_t> &d_prefix, hipStream_t st)
{
    HIPCHK(d_prefix.reserve(prefix.size()));
    HIPCHK(hipMemcpyAsync(d_prefix, prefix.data(), sizeof(int64_t) * prefix.size(), hipMemcpyHostToDevice, st));
    return 0;
}
static const size_t COMP_CAP = 16384;   // entries of a device component table ((g+1 f|f f) needs 7400)
static int upload_comp_table(int la, int lb, int lc, int ld, uint32_t *d_comp, hipStream_t st)
{
    std::vector<uint32_t> comp;
    build_comp_table(la, lb, lc, ld, comp);
    if (comp.size() > COMP_CAP) return fail("component table too large");
    HIPCHK(hipMemcpyAsync(d_comp, comp.data(), sizeof(uint32_t) * comp.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st)); // host vectors go out of scope
    return 0;
}
// the fields of EriArgs every Rys launch sets: class dimensions, the two pair lists, task prefix, component table, output
static EriArgs eri_class_args(const mi_ctx *c, int la, int lb, int lc, int ld, const PairRec *bra, const PairRec *ket, const double *prim,
                              const int64_t *prefix, int nbra, const uint32_t *comp, double *work)
{
    EriArgs E{};
    setup_eri_dims(E, la, lb, lc, ld);
    E.bra = bra; E.ket = ket; E.prim = prim; E.prefix = prefix; E.nbra = nbra;
    E.comp = comp; E.work = work; E.rys = c->rys; E.diag = 0;
    return E;
}

static int grad_records_host(mi_ctx *c);

// =================================================================================================
// mi_eri_prepare: a sequence of phases (the functions below, in call order).  What outlives the call lives in mi_ctx; what
// only the phases hand to one another travels in PrepareState.
// =================================================================================================
struct PrepareState {
    mi_ctx *c;
    hipStream_t st;
    double tol;
    int rank, nranks;
    size_t work_doubles = 0;            // capacity of the [e0|f0] hand-over buffer
    Scratch scr_work, scr_tasks;        // (returned to the per-device cache when the call ends, whichever way)
    DevBuf<uint32_t> d_comp;
    DevBuf<int64_t> d_prefix;
    double qmax = 0.0;                  // largest Schwarz factor
    std::vector<double> Qblk;           // block-pair Schwarz bounds [nbp]
    double *early_zero_ptr = nullptr;   // parked store whose zero-fill was queued early, and its size
    int64_t early_zero_doubles = 0;
    std::vector<int32_t> table;         // tile directory [nbp(nbp+1)/2] -> local tile index or -1
    int64_t off = 0;                    // doubles of the store
    int64_t nuniq = 0, nquart = 0;      // statistics: unique integrals stored, quartets evaluated
};

// ---- 1. shell pairs, primitive-pair records, transformation matrices
static int prepare_pairs(PrepareState &S)
{
    mi_ctx *c = S.c;
    const int nbas = c->nbas;
    const std::vector<std::vector<double>> c2s = c2s_tables();
    std::vector<double> &prim = c->h_prim, &Mbuf = c->h_M;
    prim.clear(); Mbuf.clear();
    c->tol = S.tol; c->grad_ready = false; c->rank = S.rank; c->nranks = S.nranks;
    c->eri_omega = c->opt_omega;   // Schwarz bounds below stay full-Coulomb (valid for erf(omega r)/r, see the header)
    for (int la = 0; la <= LMAX; la++)
        for (int lb = 0; lb <= la; lb++) {
            PairClass &P = c->pc[pc_index(la, lb)];
            P.la = la; P.lb = lb; P.ne = ne_of(la, lb); P.nsab = (2 * la + 1) * (2 * lb + 1);
        }
    for (int A = 0; A < nbas; A++)
        for (int B = 0; B <= A; B++) {
            int si = A, sj = B;
            if (c->shells[si].l < c->shells[sj].l) std::swap(si, sj);
            const ShellH &I = c->shells[si], &J = c->shells[sj];
            PairClass &P = c->pc[pc_index(I.l, J.l)];
            PairRec R;
            R.sh_i = si; R.sh_j = sj; R.ao_i = I.ao; R.ao_j = J.ao; R.pad = 0;
            R.prim_off = (int)(prim.size() / 8);
            R.nprim = append_prim_pairs(I, J, prim);
            if (R.nprim == 0) continue;
            R.m_off = (int)Mbuf.size();
            Mbuf.resize(Mbuf.size() + (size_t)2 * P.nsab * P.ne); // M [nsab][ne] followed by its transpose [ne][nsab]
            P.recs.push_back(R);
        }
    {   // HRR*c2s matrices of all pairs (OpenMP: this is the costly host part of the setup)
        std::vector<const PairRec *> all;
        for (int ci = 0; ci < NPC; ci++)
            for (const PairRec &R : c->pc[ci].recs) all.push_back(&R);
#pragma omp parallel for schedule(dynamic, 64) num_threads(host_threads())
        for (size_t q = 0; q < all.size(); q++) {
            const ShellH &I = c->shells[all[q]->sh_i], &J = c->shells[all[q]->sh_j];
            double AB[3] = {I.r[0] - J.r[0], I.r[1] - J.r[1], I.r[2] - J.r[2]};
            build_M_and_transpose(I.l, J.l, AB, c2s[I.l], c2s[J.l], Mbuf.data() + all[q]->m_off);
        }
    }
    if (Mbuf.size() > (size_t)INT32_MAX) return fail("transformation-matrix buffer exceeds 2^31 doubles");
    if (upload(&c->d_prim, prim)) return -1;
    if (upload(&c->d_M, Mbuf)) return -1;
    return 0;
}

// ---- 2. Schwarz bounds per pair (GPU)
static int prepare_schwarz(PrepareState &S)
{
    mi_ctx *c = S.c;
    hipStream_t st = S.st;
    // workspace for cartesian intermediates
    // [e0|f0] blocks travel from the Rys launch to the transform launch through this buffer: small enough that a batch written by
    // one launch is still in the 256 MiB Infinity Cache when the next reads it (`work_mb`)
    // sized to what the molecule can need (atoms of the initial guess: a few MiB), at most `work_mb`
    S.work_doubles = (size_t)8 << 17;
    const size_t cap = (size_t)std::max(8, c->opt_work_mb) << 17;
    for (int bc = 0; bc < NPC; bc++)
        for (int kc = 0; kc <= bc; kc++) {
            const PairClass &B = c->pc[bc], &Kc = c->pc[kc];
            const double need = (double)B.recs.size() * (double)Kc.recs.size() * (double)B.ne * (double)Kc.ne;
            S.work_doubles = (size_t)std::min<double>((double)cap, std::max<double>((double)S.work_doubles, need));
        }
    if (S.scr_work.ensure(c->device, SCR_EVAL_WORK, sizeof(double) * S.work_doubles)) return -1;
    HIPCHK(S.d_comp.alloc(COMP_CAP));
    double *d_work = (double *)S.scr_work.p;
    for (int ci = 0; ci < NPC; ci++) {
        PairClass &P = c->pc[ci];
        if (P.recs.empty()) continue;
        if (upload(&P.d_recs, P.recs)) return -1;
        P.q.assign(P.recs.size(), 0.0);
        HIPCHK(dev_malloc(&P.d_q, sizeof(double) * P.recs.size()));
        if (upload_comp_table(P.la, P.lb, P.la, P.lb, S.d_comp, st)) return -1;
        EriArgs E = eri_class_args(c, P.la, P.lb, P.la, P.lb, P.d_recs, P.d_recs, c->d_prim, nullptr, (int)P.recs.size(), S.d_comp, d_work);
        E.diag = 1;
        size_t per = S.work_doubles / E.ncomp;
        for (size_t b0 = 0; b0 < P.recs.size(); b0 += per) {
            int nb = (int)std::min(per, P.recs.size() - b0);
            E.t0 = (int64_t)b0; E.ntask = nb;
            if (launch_eri(c, E, nb, st)) return -1;
            SchwarzArgs A{P.d_recs + b0, c->d_M, d_work, P.ne, P.nsab, E.ncomp, P.d_q + b0};
            hipLaunchKernelGGL(schwarz_diag_kernel, dim3(nb), dim3(64), sizeof(double) * P.ne * P.ne, st, A);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipMemcpyAsync(P.q.data(), P.d_q, sizeof(double) * P.q.size(), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    for (int ci = 0; ci < NPC; ci++)
        for (double v : c->pc[ci].q) S.qmax = std::max(S.qmax, v);
    return 0;
}

// The store of the previous geometry is parked and will most likely be taken again below: its zero-fill (100 GB, 15 ms for
// ibuprofen) is queued NOW, so that it runs while the host sorts the pairs and plans tiles, runs and segments (~25 ms)
// instead of after them.  (If the parked store turns out not to fit it is freed by arena_take and the fresh one is filled.)
// ---- 3. sort pairs by q (descending), drop negligible ones; block-pair Schwarz bounds
static int prepare_sort_pairs(PrepareState &S)
{
    mi_ctx *c = S.c;
    TileArena &pk = g_arena[c->device & 15];
    if (pk.ptr && pk.doubles > 0 && !getenv("MI355_DEBUG")) {   // (the debug laps synchronise: keep their attribution)
        S.early_zero_ptr = pk.ptr; S.early_zero_doubles = pk.doubles;
        HIPCHK(hipMemsetAsync(pk.ptr, 0, sizeof(double) * (size_t)pk.doubles, S.st));
    }
    const double tol = S.tol, qmax = S.qmax;
    const int nblk = c->nblk;
    const int nbp = nblk * (nblk + 1) / 2;
    std::vector<double> &Qblk = S.Qblk;
    Qblk.assign(nbp, 0.0);
    for (int ci = 0; ci < NPC; ci++) {
        PairClass &P = c->pc[ci];
        std::vector<int> ord(P.recs.size());
        std::iota(ord.begin(), ord.end(), 0);
        // Order of the pair list.  Tasks are (bra, ket) with the ket index running fastest, and a bra only visits the leading
        // kets whose bound can survive the Schwarz test, so the list must be non-increasing in a bound.  With `ket_cluster` that
        // bound is the maximum q of the pair's CLUSTER -- the pairs whose first AOs fall into the same (block, block) pair of
        // the store -- and inside a cluster the pairs follow their AO position: kets that complete one another's 64-byte lines
        // of a tile (neighbouring k shells / l shells) are then neighbouring tasks, i.e. neighbouring lanes of the thread-per-
        // quartet kernels and neighbouring workgroups of the others (which the XCD-aware block map keeps on one L2).
        std::vector<double> cqv(P.recs.size());
        std::vector<int64_t> cid(P.recs.size(), 0);
        if (c->opt_ket_cluster) {
            std::vector<std::pair<int64_t, double>> cm;   // cluster id -> max q over the surviving pairs
            cm.reserve(P.recs.size());
            for (size_t o = 0; o < P.recs.size(); o++) {
                cid[o] = (int64_t)(P.recs[o].ao_i / BLK) * c->nblk + P.recs[o].ao_j / BLK;
                if (P.q[o] * qmax >= tol) cm.push_back({cid[o], P.q[o]});
            }
            std::sort(cm.begin(), cm.end());
            std::vector<std::pair<int64_t, double>> cmax;
            for (const auto &e : cm) { if (cmax.empty() || cmax.back().first != e.first) cmax.push_back(e); else cmax.back().second = std::max(cmax.back().second, e.second); }
            for (size_t o = 0; o < P.recs.size(); o++) {
                auto it = std::lower_bound(cmax.begin(), cmax.end(), std::make_pair(cid[o], -1.0));
                cqv[o] = (it != cmax.end() && it->first == cid[o]) ? it->second : P.q[o];
            }
            std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) {
                if (cqv[a] != cqv[b]) return cqv[a] > cqv[b];
                if (cid[a] != cid[b]) return cid[a] < cid[b];
                if (P.recs[a].ao_i != P.recs[b].ao_i) return P.recs[a].ao_i < P.recs[b].ao_i;
                return P.recs[a].ao_j < P.recs[b].ao_j;
            });
        } else {
            for (size_t o = 0; o < P.recs.size(); o++) cqv[o] = P.q[o];
            std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return P.q[a] > P.q[b]; });
        }
        std::vector<PairRec> r2;
        std::vector<double> q2, cq2;
        for (int o : ord) {
            if (P.q[o] * qmax < tol) { if (c->opt_ket_cluster) continue; else break; }
            r2.push_back(P.recs[o]);
            q2.push_back(P.q[o]);
            cq2.push_back(cqv[o]);
            const PairRec &R = P.recs[o];
            int ni = 2 * P.la + 1, nj = 2 * P.lb + 1;
            for (int I = R.ao_i / BLK; I <= (R.ao_i + ni - 1) / BLK; I++)
                for (int J = R.ao_j / BLK; J <= (R.ao_j + nj - 1) / BLK; J++) {
                    int hi = std::max(I, J), lo = std::min(I, J);
                    double &Q = Qblk[hi * (hi + 1) / 2 + lo];
                    Q = std::max(Q, P.q[o]);
                }
        }
        P.cq.swap(cq2);
        P.recs.swap(r2);
        P.q.swap(q2);
        if (upload(&P.d_recs, P.recs)) return -1;
        if (upload(&P.d_q, P.q)) return -1; // Schwarz factors in the sorted order (density-weighted screening of the gradient)
        {
            double sm = 0.0, s4 = 0.0;
            const size_t np_ = P.recs.size();
            P.max_np = 1;
            for (size_t r = 0; r < np_; r++) { sm += P.recs[r].nprim; P.max_np = std::max(P.max_np, P.recs[r].nprim); }
            for (size_t r = 0; r < np_; r += 4) {
                int mx = 0;
                for (size_t u = r; u < std::min(np_, r + 4); u++) mx = std::max(mx, P.recs[u].nprim);
                s4 += mx;
            }
            P.mean_np = np_ ? sm / np_ : 1.0;
            P.max4_np = np_ ? s4 / ((np_ + 3) / 4) : 1.0;
        }
    }
    return 0;
}

// ---- 4. tiles and runs.  Run = tiles sharing (J,K,L), ordered by I.  Runs are the sharding unit: plan_runs deals them
// to ranks longest-processing-time first by streamed bytes (every rank computes the same plan).
static int prepare_enumerate_tiles(PrepareState &S)
{
    mi_ctx *c = S.c;
    const double tol = S.tol;
    const int rank = S.rank, nranks = S.nranks;
    const int nblk = c->nblk;
    const int nbp = nblk * (nblk + 1) / 2;
    const std::vector<double> &Qblk = S.Qblk;
    auto bsize = [&](int B) { return std::min(BLK, c->nao - B * BLK); };
    c->tiles.clear(); c->tile_off.clear(); c->runs.clear();
    std::vector<int32_t> &table = S.table;
    table.assign((size_t)nbp * (nbp + 1) / 2, -1);
    int64_t nuniq = 0;
    std::vector<RunPlan> plan;
    c->tri = c->opt_tri_tiles != 0;
    plan_runs(c->nao, Qblk, S.qmax, tol, nranks, c->tri != 0, plan);
    std::vector<uint8_t> present(nranks > 1 ? table.size() : 0, 0); // sharded store: slots that live on SOME rank
    // first tile and first double of every run of this rank from the plan's counts / bytes, then the runs are filled by the
    // host threads (disjoint slices of the tile list, disjoint directory slots)
    const size_t nplan = plan.size();
    std::vector<int64_t> first_tile(nplan + 1, 0), first_off(nplan + 1, 0);
    std::vector<int> run_slot(nplan, -1);
    int nown = 0;
    for (size_t q = 0; q < nplan; q++) {
        const bool mine = plan[q].owner == rank;
        first_tile[q + 1] = first_tile[q] + (mine ? plan[q].count : 0);
        first_off[q + 1] = first_off[q] + (mine ? plan[q].bytes / 8 : 0);
        if (mine) run_slot[q] = nown++;
    }
    if (first_tile[nplan] >= INT32_MAX) return fail("too many tiles");
    c->tiles.resize((size_t)first_tile[nplan]);
    c->tile_off.resize((size_t)first_tile[nplan]);
    c->runs.resize((size_t)nown);
    int bad = 0;
#pragma omp parallel for schedule(dynamic, 256) num_threads(host_threads()) reduction(+ : nuniq) reduction(| : bad)
    for (size_t q = 0; q < nplan; q++) {
        const RunPlan &rp = plan[q];
        const int J = rp.J, K = rp.K, L = rp.L, kl = K * (K + 1) / 2 + L;
        if (rp.owner != rank) {
            for (int I = J; I < nblk; I++) {
                int ij = I * (I + 1) / 2 + J;
                if (ij >= kl && Qblk[ij] * Qblk[kl] >= tol) present[(size_t)ij * (ij + 1) / 2 + kl] = 1;
            }
            continue;
        }
        int tid = (int)first_tile[q];
        int64_t o = first_off[q];
        RunRec cur{J, K, L, tid, 0};
        for (int I = J; I < nblk; I++) {
            int ij = I * (I + 1) / 2 + J;
            if (ij < kl) continue;
            if (Qblk[ij] * Qblk[kl] < tol) continue;
            table[(size_t)ij * (ij + 1) / 2 + kl] = (int32_t)tid;
            c->tiles[tid] = {I, J, K, L};
            c->tile_off[tid] = o;
            int bi = bsize(I), bj = bsize(J), bk = bsize(K), bl = bsize(L);
            o += tile_doubles_padded(c->tri && I == J, c->tri && K == L, bi, bk); // j is always padded to 8 rows (J==last implies I==last: rare)
            int64_t nij = (I > J) ? (int64_t)bi * bj : (int64_t)bi * (bi + 1) / 2;
            int64_t nkl = (K > L) ? (int64_t)bk * bl : (int64_t)bk * (bk + 1) / 2;
            nuniq += (ij > kl) ? nij * nkl : nij * (nij + 1) / 2;
            cur.count++; tid++;
        }
        if (cur.count != rp.count || o != first_off[q + 1]) bad |= 1;
        c->runs[run_slot[q]] = cur;
    }
    if (bad) return fail("internal: run plan / tile enumeration mismatch");
    S.off = first_off[nplan];
    S.nuniq = nuniq;
    if (c->d_tile_present) { dev_free(c->d_tile_present); c->d_tile_present = nullptr; }
    if (nranks > 1 && upload(&c->d_tile_present, present)) return -1;
    c->n_tiles = (int64_t)c->tiles.size();
    c->tile_doubles = S.off;
    if (c->n_tiles >= INT32_MAX) return fail("too many tiles");
    return 0;
}

static int prepare_upload_directory(PrepareState &S)
{
    mi_ctx *c = S.c;
    if (upload(&c->d_tile_table, S.table)) return -1;
    if (upload(&c->d_tile_off, c->tile_off)) return -1;
    std::vector<int> tI(c->tiles.size());
    for (size_t i = 0; i < tI.size(); i++) tI[i] = c->tiles[i].I;
    if (upload(&c->d_tile_I, tI)) return -1;
    if (upload(&c->d_runs, c->runs)) return -1;
    return 0;
}

// J/K work items ("segments"): runs cut into chunks; either one wave per item (longest first, the
// hardware dispatcher balances) or a fixed number of waves with equal-cost contiguous shares.
static int prepare_jk_segments(PrepareState &S)
{
    mi_ctx *c = S.c;
    const int64_t off = S.off;
    auto tile_cost = [&](int tid) {
        int64_t nd = (tid + 1 < (int)c->tile_off.size() ? c->tile_off[tid + 1] : off) - c->tile_off[tid];
        return (double)nd * 8.0 + 8192.0; // streamed bytes + fixed per-tile overhead
    };
    const int chunk = c->opt_runmax > 0 ? c->opt_runmax : (int)std::min<int64_t>(64, std::max<int64_t>(8, c->n_tiles / 2048));
    std::vector<RunRec> segs;
    std::vector<int> wave_seg;
    int nw, w = 0;
    c->n_jk_cached = 0;   // (the cached prefix exists for the longest-first order only)
    if (c->opt_jk_waves <= 0) {
        for (const RunRec &r : c->runs)
            for (int t0 = 0; t0 < r.count; t0 += chunk) segs.push_back(RunRec{r.J, r.K, r.L, r.first + t0, std::min(chunk, r.count - t0)});
        std::vector<double> cost(segs.size(), 0.0);
#pragma omp parallel for schedule(static) num_threads(host_threads())
        for (size_t q = 0; q < segs.size(); q++)
            for (int t = 0; t < segs[q].count; t++) cost[q] += tile_cost(segs[q].first + t);
        std::vector<int> ord(segs.size());
        std::iota(ord.begin(), ord.end(), 0);
        std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return cost[a] > cost[b]; });
        std::vector<RunRec> sorted(segs.size());
        for (size_t q = 0; q < segs.size(); q++) sorted[q] = segs[ord[q]];
        segs.swap(sorted);
        if (off * 8 > ((int64_t)256 << 20) && c->opt_jk_cache_mb > 0) {
            double acc_b = 0.0;
            const double lim = (double)c->opt_jk_cache_mb * 1048576.0;
            std::vector<double> sc(segs.size(), 0.0);
#pragma omp parallel for schedule(static) num_threads(host_threads())
            for (size_t q = 0; q < segs.size(); q++)
                for (int t = 0; t < segs[q].count; t++) sc[q] += tile_cost(segs[q].first + t) - 8192.0;
            while (c->n_jk_cached < (int)segs.size() && acc_b + sc[c->n_jk_cached] <= lim) acc_b += sc[c->n_jk_cached++];
        }
        nw = (int)segs.size();
        wave_seg.resize(nw + 1);
        std::iota(wave_seg.begin(), wave_seg.end(), 0);
        w = nw - 1;
    } else {
        nw = (int)std::min<int64_t>(c->opt_jk_waves, std::max<int64_t>(c->n_tiles, 1));
        wave_seg.assign(nw + 1, 0);
        double total_cost = 0.0;
        for (int tid = 0; tid < (int)c->n_tiles; tid++) total_cost += tile_cost(tid);
        double per = total_cost / nw, acc_cost = 0.0;
        for (const RunRec &r : c->runs) {
            RunRec cur{r.J, r.K, r.L, r.first, 0};
            for (int t = 0; t < r.count; t++) {
                int tid = r.first + t;
                double tc = tile_cost(tid);
                int wt = std::min(nw - 1, (int)((acc_cost + 0.5 * tc) / per));
                acc_cost += tc;
                if (wt != w) {
                    if (cur.count) segs.push_back(cur);
                    for (int x = w + 1; x <= wt; x++) wave_seg[x] = (int)segs.size();
                    w = wt;
                    cur = RunRec{r.J, r.K, r.L, tid, 0};
                }
                cur.count++;
            }
            if (cur.count) segs.push_back(cur);
        }
    }
    for (int x = w + 1; x <= nw; x++) wave_seg[x] = (int)segs.size();
    c->n_jk_waves = nw;
    c->n_jk_segs = (int)segs.size();
    if (getenv("MI355_DEBUG")) {
        int mx = 0, mn = 1 << 30, maxseg = 0;
        for (int x = 0; x < nw; x++) {
            int nt = 0;
            for (int sgi = wave_seg[x]; sgi < wave_seg[x + 1]; sgi++) nt += segs[sgi].count;
            mx = std::max(mx, nt); mn = std::min(mn, nt); maxseg = std::max(maxseg, wave_seg[x + 1] - wave_seg[x]);
        }
        fprintf(stderr, "[mi355] tiles=%ld runs=%zu segs=%zu waves=%d tiles/wave min=%d max=%d maxsegs/wave=%d\n",
                (long)c->n_tiles, c->runs.size(), segs.size(), nw, mn, mx, maxseg);
    }
    if (upload(&c->d_segs, segs)) return -1;
    if (upload(&c->d_wave_seg, wave_seg)) return -1;
    return 0;
}

// The store itself: a host-side decision first (MI_ERR_NOMEM before anything is allocated; sizes: mi_eri_get_memory), then the
// parked store of the previous geometry or a fresh allocation, zero-filled unless prepare_sort_pairs queued that already
static int prepare_allocate_store(PrepareState &S)
{
    mi_ctx *c = S.c;
    const int64_t off = S.off;
    size_t freeb = 0, totb = 0;
    HIPCHK(hipMemGetInfo(&freeb, &totb));
    freeb += (size_t)g_arena[c->device & 15].doubles * 8; // a parked store is reusable (or freed) by arena_take
    freeb += pool_parked_bytes(c->device);                // ... and so are the pool's parked blocks
    c->mem_need_bytes = (int64_t)off * 8;
    c->mem_free_bytes = (int64_t)freeb;
    if ((size_t)off * 8 + ((size_t)1 << 30) > freeb) {
        fail("resident ERI store needs %.1f GB but only %.1f GB of HBM is free; shard over more GPUs",
             off * 8e-9, freeb * 1e-9);
        return MI_ERR_NOMEM; // sizes: mi_eri_get_memory
    }
    c->tile_alloc = std::max<int64_t>(off, 1);
    {
        TileArena &pk = g_arena[c->device & 15];
        if (pk.ptr && pk.doubles >= c->tile_alloc && pk.doubles <= c->tile_alloc + c->tile_alloc / 4 + (1 << 20)) c->tile_alloc = pk.doubles;
        else {
            // a fresh allocation: 2 % of head room, so that the next geometry of an optimisation (a few more tiles survive the
            // Schwarz test) still fits the parked store -- re-allocating 103 GB took 6 s on a box of the pool (measured in a
            // geometry step of ibuprofen/def2-TZVP: 7.6 s instead of 1.9 s)
            const int64_t padded = c->tile_alloc + c->tile_alloc / 50;
            if ((size_t)padded * 8 + ((size_t)1 << 30) <= freeb) c->tile_alloc = padded;
        }
    }
    if (arena_take(c->device, c->tile_alloc, &c->d_tiles)) return -1;
    if (!(c->d_tiles == S.early_zero_ptr && off <= S.early_zero_doubles))
        HIPCHK(hipMemsetAsync(c->d_tiles, 0, sizeof(double) * std::max<int64_t>(off, 1), S.st));
    return 0;
}

// ---- 5. evaluate every Schwarz-surviving canonical shell quartet, class by class.  One (bra class, ket class) pair is set
// up once (ClassPairEval) and offered to three routes in turn; each returns 1 (handled), 0 (not its class) or -1 (error).
struct ClassPairEval {
    const PairClass *B, *Kc;
    int64_t ntask;
    EriArgs E;
    XfArgs X;
    size_t shm2;              // LDS of the transform kernel per quartet
    bool xf_mfma, xf_small;   // transform kernel: MFMA tiles / four quartets per wave
    unsigned xcd_wave, xcd_tpq;
    bool dbg;                 // MI355_DEBUG=2: per-class timing
};
static int eval_route_tpq(PrepareState &S, const ClassPairEval &P);
static int eval_route_fused(PrepareState &S, const ClassPairEval &P);
static int eval_route_two_launch(PrepareState &S, ClassPairEval &P);

static int prepare_evaluate_class_pair(PrepareState &S, PairClass &B, PairClass &Kc, bool same)
{
    mi_ctx *c = S.c;
    hipStream_t st = S.st;
    const double tol = S.tol;
    const int nranks = S.nranks;
    double *d_work = (double *)S.scr_work.p;
    std::vector<int64_t> prefix;
    const int64_t ntask = class_prefix(B, Kc, same, tol, prefix);
    if (ntask == 0) return 0;
    S.nquart += ntask;
    if (prefix_to_device(prefix, S.d_prefix, st)) return -1;
    const int64_t *d_prefix = S.d_prefix;
    ClassPairEval P{};
    P.B = &B; P.Kc = &Kc; P.ntask = ntask;
    const bool tpq_class = c->opt_eri_tpq && B.mean_np * Kc.mean_np <= c->opt_tpq_maxprim && ntask >= c->opt_tpq_min_tasks &&
                           tpq_has_class(B.la, B.lb, Kc.la, Kc.lb);
    const TaskIdx *d_tasks = nullptr;
    if (c->opt_task_table && !tpq_class && ntask >= 65536) {   // the wave-per-quartet pair walks the task list twice
        if (S.scr_tasks.ensure(c->device, SCR_EVAL_TASKS, sizeof(TaskIdx) * (size_t)ntask)) return -1;
        hipLaunchKernelGGL(fill_tasks_kernel, dim3((unsigned)((ntask + 255) / 256)), dim3(256), 0, st, d_prefix, (int)B.recs.size(), ntask,
                           (TaskIdx *)S.scr_tasks.p);
        d_tasks = (const TaskIdx *)S.scr_tasks.p;
    }
    if (upload_comp_table(B.la, B.lb, Kc.la, Kc.lb, S.d_comp, st)) return -1;
    EriArgs &E = P.E;
    E = eri_class_args(c, B.la, B.lb, Kc.la, Kc.lb, B.d_recs, Kc.d_recs, c->d_prim, d_prefix, (int)B.recs.size(), S.d_comp, d_work);
    E.tasks = d_tasks;
    E.omega = c->eri_omega;
    E.ni = 2 * B.la + 1; E.nj = 2 * B.lb + 1; E.nk = 2 * Kc.la + 1; E.nl = 2 * Kc.lb + 1;
    E.own_table = nranks > 1 ? c->d_tile_table : nullptr;
    E.h_shared_np = B.mean_np; E.h_vary_mean = Kc.mean_np; E.h_vary_max4 = Kc.max4_np;
    E.scr.q_bra = B.d_q; E.scr.q_ket = Kc.d_q; E.qtol = c->opt_ket_cluster ? tol : 0.0;
    E.prim_lds = (c->opt_prim_lds && B.max_np + Kc.max_np <= 160) ? B.max_np + Kc.max_np : 0;
    P.xcd_wave = c->opt_xcd_map ? 32u : 0u; P.xcd_tpq = c->opt_xcd_map ? 8u : 0u;
    E.xcd = P.xcd_wave;
    XfArgs &X = P.X;
    X.bra = B.d_recs; X.ket = Kc.d_recs; X.Mbuf = c->d_M; X.prefix = d_prefix; X.nbra = E.nbra;
    X.ne = B.ne; X.nf = Kc.ne; X.nsab = B.nsab; X.nscd = Kc.nsab; X.nsb = 2 * B.lb + 1; X.nsd = 2 * Kc.lb + 1;
    X.work = d_work; X.ncomp = E.ncomp; X.tile_table = c->d_tile_table; X.tile_off = c->d_tile_off;
    X.tiles = c->d_tiles; X.nao = c->nao; X.tri = c->tri;
    X.check_owner = nranks > 1; X.ni = E.ni; X.nj = E.nj; X.nk = E.nk; X.nl = E.nl;
    X.q_bra = E.scr.q_bra; X.q_ket = E.scr.q_ket; X.qtol = E.qtol; X.xcd = P.xcd_wave; X.tasks = E.tasks;
    P.shm2 = sizeof(double) * ((size_t)X.ne * X.nf + (size_t)X.nsab * X.nf);
    {
        const size_t with_m = P.shm2 + sizeof(double) * ((size_t)2 * X.nsab * X.ne + (size_t)2 * X.nscd * X.nf);
        X.m_lds = (c->opt_xf_mlds && with_m <= (size_t)c->opt_xf_mlds * 1024) ? 1 : 0;
        if (X.m_lds) P.shm2 = with_m;
    }
    // matrix-core path only for the large classes: below, the lean per-lane kernel (56 VGPRs, 8 waves per SIMD) hides the
    // per-quartet latency chain better than MFMA tiles at 3-4 waves per SIMD (measured per class on ibuprofen/def2-TZVP)
    P.xf_mfma = (mfma_worthwhile(X.nsab, X.nf, X.ne) || mfma_worthwhile(X.nsab, X.nscd, X.nf)) && X.nsab * X.nscd >= c->opt_xf_mfma_min;
    P.xf_small = !P.xf_mfma && X.nsab * X.nscd <= c->opt_xf_qpw_max && P.shm2 * 4 <= 64 * 1024; // four quartets per wave
    if (P.shm2 > 64 * 1024)
        HIPCHK(hipFuncSetAttribute(P.xf_mfma ? (const void *)eri_transform_scatter<true, 64> : (const void *)eri_transform_scatter<false, 64>,
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.shm2));
    P.dbg = getenv("MI355_DEBUG") != nullptr && getenv("MI355_DEBUG")[0] == '2';
    int used = eval_route_tpq(S, P);
    if (!used) used = eval_route_fused(S, P);
    if (!used) used = eval_route_two_launch(S, P);
    return used < 0 ? -1 : 0;
}

// low angular classes: one thread per quartet, fused Rys + HRR + cart->sph + scatter (eri_tpq_kernel)
// ... when the contraction is shallow enough: a thread walks ALL primitive quartets of its shell quartet, so deeply
// contracted shells (cc-pVXZ s shells: hundreds of primitive quartets) serialise and the wave-per-quartet path, which
// spreads them over lanes, wins (measured: benzene/cc-pVTZ 54 vs 63 ms, ibuprofen/def2-TZVP 0.40 vs 0.29 s)
static int eval_route_tpq(PrepareState &S, const ClassPairEval &P)
{
    mi_ctx *c = S.c;
    hipStream_t st = S.st;
    const PairClass &B = *P.B, &Kc = *P.Kc;
    const EriArgs &E = P.E;
    const int64_t ntask = P.ntask;
    if (!(c->opt_eri_tpq && B.mean_np * Kc.mean_np <= c->opt_tpq_maxprim && ntask >= c->opt_tpq_min_tasks)) return 0;
    TpqArgs Q{};
    Q.bra = B.d_recs; Q.ket = Kc.d_recs; Q.prim = c->d_prim; Q.prefix = E.prefix; Q.nbra = E.nbra; Q.t0 = 0; Q.ntask = ntask;
    Q.c2s = c->d_c2s;
    for (int q = 0; q <= LMAX + 1; q++) Q.c2s_off[q] = c->c2s_off[q];
    Q.rys = c->rys; Q.X = P.X; Q.shell_xyz = c->d_shell_xyz; Q.check_owner = S.nranks > 1;
    Q.q_bra = E.scr.q_bra; Q.q_ket = E.scr.q_ket; Q.qtol = E.qtol; Q.xcd = P.xcd_tpq; Q.omega = E.omega;
    auto ta = std::chrono::steady_clock::now();
    if (P.dbg) hipStreamSynchronize(st);
    const int used = launch_eri_tpq(B.la, B.lb, Kc.la, Kc.lb, Q, st);
    if (used > 0 && P.dbg) {
        hipStreamSynchronize(st);
        const double t_rys = std::chrono::duration<double>(std::chrono::steady_clock::now() - ta).count();
        fprintf(stderr, "[mi355] eri class (%d%d|%d%d): %ld quartets, thread-per-quartet fused kernel %.4f s (%.2f ns/q)\n", B.la, B.lb,
                Kc.la, Kc.lb, (long)ntask, t_rys, t_rys / ntask * 1e9);
    }
    return used;
}

// (option eri_fused) one fused launch per (at most 2^30) tasks: no hand-over buffer, so no batching by its size
static int eval_route_fused(PrepareState &S, const ClassPairEval &P)
{
    mi_ctx *c = S.c;
    hipStream_t st = S.st;
    const PairClass &B = *P.B, &Kc = *P.Kc;
    const EriArgs &E = P.E;
    const XfArgs &X = P.X;
    const int64_t ntask = P.ntask;
    if (!(c->opt_eri_fused && !E.diag)) return 0;
    FusedArgs F;
    F.R = E; F.X = X;
    F.R.PB = std::max(1, std::min(E.PB, B.max_np * Kc.max_np));   // uncontracted d / f shells: one primitive quartet per batch
    F.R.prim_lds = 0; F.R.own_table = nullptr; F.R.qtol = 0.0; F.R.scr.dmax = nullptr;   // (the transform half screens: check_owner, qtol)
    F.X.m_lds = 0;
    const size_t scratch = RysLds{F.R.PB, E.nroots, E.tsz}.doubles();
    const size_t shmf = sizeof(double) * ((size_t)X.ne * X.nf + std::max((size_t)X.nsab * X.nf, scratch));
    if (shmf > 160 * 1024) return 0;
    const int perlane = (E.ncomp + 63) / 64;
    auto ta = std::chrono::steady_clock::now();
    if (P.dbg) hipStreamSynchronize(st);
    for (int64_t t0 = 0; t0 < ntask; t0 += (int64_t)1 << 30) {
        const int64_t nb = std::min<int64_t>((int64_t)1 << 30, ntask - t0);
        F.X.t0 = t0; F.X.ntask = nb; F.X.xcd = nb >= 2048 ? P.xcd_wave : 0u;
        const dim3 grid(eri_grid(nb, F.X.xcd));
#define FUSED_LAUNCH(MF, MC)                                                                                                               \
    do {                                                                                                                                   \
        if (shmf > 64 * 1024) HIPCHK(hipFuncSetAttribute((const void *)eri_fused_kernel<MF, MC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmf)); \
        hipLaunchKernelGGL((eri_fused_kernel<MF, MC>), grid, dim3(64), shmf, st, F);                                                        \
    } while (0)
        if (P.xf_mfma) {
            if (perlane <= 4) FUSED_LAUNCH(true, 4); else if (perlane <= 16) FUSED_LAUNCH(true, 16); else FUSED_LAUNCH(true, 32);
        } else {
            if (perlane <= 1) FUSED_LAUNCH(false, 1); else if (perlane <= 4) FUSED_LAUNCH(false, 4);
            else if (perlane <= 16) FUSED_LAUNCH(false, 16); else FUSED_LAUNCH(false, 32);
        }
#undef FUSED_LAUNCH
        HIPCHK(hipGetLastError());
    }
    if (P.dbg) {
        hipStreamSynchronize(st);
        const double t_rys = std::chrono::duration<double>(std::chrono::steady_clock::now() - ta).count();
        fprintf(stderr, "[mi355] eri class (%d%d|%d%d): %ld quartets, fused rys+transform+scatter %.4f s (%.2f ns/q)\n", B.la, B.lb,
                Kc.la, Kc.lb, (long)ntask, t_rys, t_rys / ntask * 1e9);
    }
    return 1;
}

// everything else: Rys launch -> hand-over buffer -> transform + scatter launch, in batches of what the buffer holds
static int eval_route_two_launch(PrepareState &S, ClassPairEval &P)
{
    mi_ctx *c = S.c;
    hipStream_t st = S.st;
    const PairClass &B = *P.B, &Kc = *P.Kc;
    EriArgs &E = P.E;
    XfArgs &X = P.X;
    const int64_t ntask = P.ntask;
    const size_t shm2 = P.shm2;
    const bool dbg = P.dbg;
    double t_rys = 0.0, t_xf = 0.0;
    const int64_t per = std::min<int64_t>((int64_t)(S.work_doubles / E.ncomp), (int64_t)1 << 24);
    for (int64_t t0 = 0; t0 < ntask; t0 += per) {
        int nb = (int)std::min<int64_t>(per, ntask - t0);
        E.t0 = t0; E.ntask = nb; X.t0 = t0;
        auto ta = std::chrono::steady_clock::now();
        if (dbg) hipStreamSynchronize(st);
        if (launch_eri(c, E, nb, st)) return -1;
        if (dbg) { hipStreamSynchronize(st); t_rys += std::chrono::duration<double>(std::chrono::steady_clock::now() - ta).count(); ta = std::chrono::steady_clock::now(); }
        X.ntask = nb;
        X.xcd = nb >= 2048 ? P.xcd_wave : 0u;
        E.xcd = P.xcd_wave;   // (launch_eri switches the map off for small launches)
        if (P.xf_mfma) hipLaunchKernelGGL((eri_transform_scatter<true, 64>), dim3(eri_grid(nb, X.xcd)), dim3(64), shm2, st, X);
        else if (P.xf_small) hipLaunchKernelGGL((eri_transform_scatter<false, 16>), dim3(eri_grid((nb + 3) / 4, X.xcd)), dim3(64), shm2 * 4, st, X);
        else hipLaunchKernelGGL((eri_transform_scatter<false, 64>), dim3(eri_grid(nb, X.xcd)), dim3(64), shm2, st, X);
        HIPCHK(hipGetLastError());
        if (dbg) { hipStreamSynchronize(st); t_xf += std::chrono::duration<double>(std::chrono::steady_clock::now() - ta).count(); }
    }
    if (dbg)
        fprintf(stderr, "[mi355] eri class (%d%d|%d%d): %ld quartets, rys %.4f s (%.2f ns/q), transform+scatter %.4f s (%.2f ns/q)\n", B.la, B.lb,
                Kc.la, Kc.lb, (long)ntask, t_rys, t_rys / ntask * 1e9, t_xf, t_xf / ntask * 1e9);
    return 1;
}

static int prepare_evaluate(PrepareState &S)
{
    mi_ctx *c = S.c;
    for (int bc = 0; bc < NPC; bc++)
        for (int kc = 0; kc <= bc; kc++) {
            PairClass &B = c->pc[bc], &Kc = c->pc[kc];
            if (B.recs.empty() || Kc.recs.empty()) continue;
            if (prepare_evaluate_class_pair(S, B, Kc, bc == kc)) return -1;
        }
    HIPCHK(hipStreamSynchronize(S.st));
    return 0;
}

extern "C" int mi_eri_prepare(mi_ctx *c, double tol, int rank, int nranks, void *stream)
{
    if (c && check_orbital_lmax(c, "mi_eri_prepare")) return -1;
    if (!c) return fail("mi_eri_prepare: null context");
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail("mi_eri_prepare: bad rank/nranks");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    auto t_start = std::chrono::steady_clock::now();
    auto t_phase = t_start;
    auto lap = [&](const char *what) {
        if (!getenv("MI355_DEBUG")) return;
        hipStreamSynchronize(st);
        auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[mi355] eri_prepare %-28s %.3f s\n", what, std::chrono::duration<double>(now - t_phase).count());
        t_phase = now;
    };
    free_eri(c);
    if (set_tile_order(c, c->opt_ao_order ? 1 : 0)) return -1;
    PrepareState S;
    S.c = c; S.tol = tol; S.rank = rank; S.nranks = nranks; S.st = st;
    if (prepare_pairs(S)) return -1;
    lap("pairs + M matrices");
    if (prepare_schwarz(S)) return -1;
    lap("schwarz");
    if (prepare_sort_pairs(S)) return -1;
    lap("sort pairs");
    if (prepare_enumerate_tiles(S)) return -1;
    lap("  plan + tile enumeration");
    if (prepare_upload_directory(S)) return -1;
    lap("  directory uploads");
    if (prepare_jk_segments(S)) return -1;
    lap("  J/K segments");
    if (int rc = prepare_allocate_store(S)) return rc;   // -1, or MI_ERR_NOMEM: the caller shards or goes direct
    lap("tiles/runs/segments + alloc");
    if (prepare_evaluate(S)) return -1;
    lap("quartet evaluation");
    S.d_prefix.reset(); S.d_comp.reset();
    S.scr_work.release(); S.scr_tasks.release();
    lap("free scratch");
    c->stats.n_tiles = c->n_tiles;
    c->stats.n_runs = (int64_t)c->runs.size();
    c->stats.stored_bytes = S.off * 8;
    c->stats.n_unique_eri = S.nuniq;
    c->stats.n_quartets = S.nquart;
    c->stats.seconds_eri = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    c->eri_ready = true;
    if (c->opt_grad_prefetch) {
        c->grad_host_rc = 0;
        c->grad_worker = std::thread([c]() {
            c->grad_host_rc = grad_records_host(c);
            if (c->grad_host_rc) c->grad_host_err = mi_last_error();   // (thread-local error string of the helper)
        });
    }
    return 0;
}

// Schwarz factors q[ish][jsh] = sqrt(max |(ab|ab)|) of the shell pairs kept by the last mi_eri_prepare (0 for pairs dropped
// as negligible: q * q_max < tol), host array [nbas][nbas] (tests: against the oracle's restatement of CVHFnr_int2e_q_cond).
extern "C" int mi_schwarz_get(const mi_ctx *c, double *q)
{
    if (!c || !q) return fail("mi_schwarz_get: null argument");
    if (!c->eri_ready) return fail("mi_schwarz_get: call mi_eri_prepare first");
    std::fill(q, q + (size_t)c->nbas * c->nbas, 0.0);
    for (int ci = 0; ci < NPC; ci++) {
        const PairClass &P = c->pc[ci];
        for (size_t r = 0; r < P.recs.size(); r++) {
            q[(size_t)P.recs[r].sh_i * c->nbas + P.recs[r].sh_j] = P.q[r];
            q[(size_t)P.recs[r].sh_j * c->nbas + P.recs[r].sh_i] = P.q[r];
        }
    }
    return 0;
}

extern "C" int mi_eri_get_memory(const mi_ctx *c, int64_t *need_bytes, int64_t *free_bytes)
{
    if (!c || !need_bytes || !free_bytes) return fail("mi_eri_get_memory: null argument");
    *need_bytes = c->mem_need_bytes;
    *free_bytes = c->mem_free_bytes;
    return 0;
}

// =================================================================================================
// Density fitting: three-index (ij|P) and two-index (P|Q) Coulomb integrals over an auxiliary
// basis with the SAME Rys kernels -- an auxiliary function P is handled as the "shell pair" (P, unit s function), i.e. a
// four-centre quartet (ij|P 1).  Stands in for libcint int3c2e_sph / int2c2e_sph behind `mf.density_fit()` [MEM]; the
// contractions with the density (J, K) are dense FP64 GEMMs done by the caller.
// `aux` is an ordinary context built from the auxiliary basis whose LAST shell is the unit function: an s primitive with
// exponent 0 and coefficient sqrt(4 pi) (so that coefficient * Y_00 = 1).
// d_int3c: [nao][nao][naux] (both (i,j) and (j,i) written), d_int2c: [naux][naux]; either may be NULL.
// =================================================================================================
struct DfPairs {
    std::vector<PairRec> recs[NPC];       // orbital shell pairs by class
    std::vector<PairRec> aux[LMAX + 1];   // (P, unit) "pairs" by l_P
    std::vector<double> prim, Mbuf;
};

extern "C" int mi_df_build(mi_ctx *c, mi_ctx *aux, double *d_int3c, double *d_int2c, void *stream)
{
    if (!c || !aux) return fail("mi_df_build: null context");
    if (c->opt_omega != 0.0 || c->eri_omega != 0.0 || aux->opt_omega != 0.0 || aux->eri_omega != 0.0)
        return fail("mi_df_build: density fitting of long-range (omega != 0) integrals is not implemented");
    if (aux->nbas < 2) return fail("mi_df_build: the auxiliary context needs at least one function plus the unit shell");
    const ShellH &U = aux->shells.back();
    if (U.l != 0 || U.nprim != 1 || U.exps[0] != 0.0) return fail("mi_df_build: the last auxiliary shell must be the unit s function (exponent 0)");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    const int naux = aux->nao - 1, unit_ao = aux->nao - 1, nP = aux->nbas - 1;
    const std::vector<std::vector<double>> c2s = c2s_tables();
    DfPairs D;
    // orbital pairs (as in mi_eri_prepare step 1, no Schwarz sorting: every pair is fitted)
    for (int A = 0; A < c->nbas; A++)
        for (int B = 0; B <= A; B++) {
            int si = A, sj = B;
            if (c->shells[si].l < c->shells[sj].l) std::swap(si, sj);
            const ShellH &I = c->shells[si], &J = c->shells[sj];
            double AB[3] = {I.r[0] - J.r[0], I.r[1] - J.r[1], I.r[2] - J.r[2]};
            PairRec R{si, sj, I.ao_nat, J.ao_nat, (int)(D.prim.size() / 8), 0, 0, 0};   // dense output in the caller's AO order
            R.nprim = append_prim_pairs(I, J, D.prim);
            if (R.nprim == 0) continue;
            R.m_off = (int)D.Mbuf.size();
            D.Mbuf.resize(D.Mbuf.size() + (size_t)2 * (2 * I.l + 1) * (2 * J.l + 1) * ne_of(I.l, J.l));
            build_M_and_transpose(I.l, J.l, AB, c2s[I.l], c2s[J.l], D.Mbuf.data() + R.m_off);
            D.recs[pc_index(I.l, J.l)].push_back(R);
        }
    // auxiliary "pairs" (P, unit)
    for (int Pn = 0; Pn < nP; Pn++) {
        const ShellH &S = aux->shells[Pn];
        PairRec R{Pn, aux->nbas - 1, S.ao_nat, unit_ao, (int)(D.prim.size() / 8), S.nprim, 0, 0};
        D.prim.resize(D.prim.size() + (size_t)8 * S.nprim);
        write_aux_prims(S, U, D.prim.data() + (size_t)8 * R.prim_off);
        double AB[3] = {0.0, 0.0, 0.0};
        R.m_off = (int)D.Mbuf.size();
        D.Mbuf.resize(D.Mbuf.size() + (size_t)2 * (2 * S.l + 1) * ncart(S.l));
        build_M_and_transpose(S.l, 0, AB, c2s[S.l], c2s[0], D.Mbuf.data() + R.m_off);
        // c2s of the unit function: build_M multiplied by c2s[0] = 1/sqrt(4 pi); its coefficient sqrt(4 pi) restores 1
        D.aux[S.l].push_back(R);
    }
    if (D.Mbuf.size() > (size_t)INT32_MAX) return fail("mi_df_build: transformation-matrix buffer exceeds 2^31 doubles");
    DevBuf<double> d_prim, d_M, d_work;
    DevBuf<uint32_t> d_comp;
    DevBuf<int64_t> d_prefix;
    DevBuf<PairRec> d_rec_o[NPC], d_rec_a[LMAX + 1];
    if (d_prim.upload(D.prim) || d_M.upload(D.Mbuf)) return -1;
    for (int q = 0; q < NPC; q++) if (!D.recs[q].empty() && d_rec_o[q].upload(D.recs[q])) return -1;
    for (int l = 0; l <= LMAX; l++) if (!D.aux[l].empty() && d_rec_a[l].upload(D.aux[l])) return -1;
    const size_t WORK_DOUBLES = (size_t)32 << 20;
    HIPCHK(d_work.alloc(WORK_DOUBLES));
    HIPCHK(d_comp.alloc(COMP_CAP));
    // one pass per (bra class, auxiliary l): bra = orbital pairs (3-index) or auxiliary pairs (2-index)
    auto run = [&](const PairRec *d_bra, int nbra, int la, int lb, int lk, int mode, double *out, int ld_nao) -> int {
        const int nket = (int)D.aux[lk].size();
        if (nbra == 0 || nket == 0) return 0;
        std::vector<int64_t> prefix;
        const int64_t ntask = dense_prefix(nbra, nket, prefix);
        if (prefix_to_device(prefix, d_prefix, st)) return -1;
        if (upload_comp_table(la, lb, lk, 0, d_comp, st)) return -1;
        EriArgs E = eri_class_args(c, la, lb, lk, 0, d_bra, d_rec_a[lk], d_prim, d_prefix, nbra, d_comp, d_work);
        E.ni = 2 * la + 1; E.nj = 2 * lb + 1; E.nk = 2 * lk + 1; E.nl = 1;
        XfArgs X{};
        X.bra = d_bra; X.ket = d_rec_a[lk]; X.Mbuf = d_M; X.prefix = d_prefix; X.nbra = nbra;
        X.ne = ne_of(la, lb); X.nf = ncart(lk); X.nsab = (2 * la + 1) * (2 * lb + 1); X.nscd = 2 * lk + 1; X.nsb = 2 * lb + 1; X.nsd = 1;
        X.work = d_work; X.ncomp = E.ncomp; X.nao = ld_nao; X.check_owner = 0;
        X.ni = E.ni; X.nj = E.nj; X.nk = E.nk; X.nl = 1;
        X.dense_out = out; X.dense_mode = mode; X.dense_n = naux;
        const size_t shm2 = sizeof(double) * ((size_t)X.ne * X.nf + (size_t)X.nsab * X.nf);
        int64_t per = std::min<int64_t>((int64_t)(WORK_DOUBLES / E.ncomp), (int64_t)1 << 22);
        if (c->opt_df_batch_max > 0) per = std::min<int64_t>(per, c->opt_df_batch_max);
        for (int64_t t0 = 0; t0 < ntask; t0 += per) {
            const int nb = (int)std::min<int64_t>(per, ntask - t0);
            E.t0 = t0; E.ntask = nb; X.t0 = t0; X.ntask = nb;
            if (launch_eri(c, E, nb, st)) return -1;
            hipLaunchKernelGGL((eri_transform_scatter<false, 64>), dim3(nb), dim3(64), shm2, st, X);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipStreamSynchronize(st));
        return 0;
    };
    int rc = 0;
    if (d_int3c)
        for (int la = 0; la <= LMAX && !rc; la++)
            for (int lb = 0; lb <= la && !rc; lb++)
                for (int lk = 0; lk <= LMAX && !rc; lk++) {
                    const int q = pc_index(la, lb);
                    rc = run(d_rec_o[q], (int)D.recs[q].size(), la, lb, lk, 1, d_int3c, c->nao);
                }
    if (d_int2c)
        for (int lp = 0; lp <= LMAX && !rc; lp++)
            for (int lk = 0; lk <= LMAX && !rc; lk++) rc = run(d_rec_a[lp], (int)D.aux[lp].size(), lp, 0, lk, 2, d_int2c, naux);
    return rc;
}

extern "C" int mi_eri_get_stats(const mi_ctx *c, mi_eri_stats *out)
{
    if (!c || !out) return fail("mi_eri_get_stats: null argument");
    *out = c->stats;
    return 0;
}

// =================================================================================================
// J/K digestion of the resident tiles.
//
// One wave per run (tiles sharing J,K,L; I varies).  Lane (i,k) = (lane>>3, lane&7) owns the 8x8
// (j,l) sub-block T[i,:,k,:] of each tile and performs all six contractions per loaded value:
//   per tile  : K_IK (in-lane), J_IJ and K_IL (reduce over the 8 k-lanes)
//   per run   : J_KL and K_JK (reduce over the 8 i-lanes), K_JL (reduce over all 64 lanes)
// Partial blocks are added with FP64 global atomics into padded accumulators; the finalize kernel
// forms J = 2 (Jacc + Jacc^T), K = Kacc + Kacc^T (tile values are pre-weighted, see put_tile).
// =================================================================================================
typedef double d2_t __attribute__((ext_vector_type(2)));

// The resident tile store as its streaming kernels see it (J/K, batched J/K, quarter transformation): the first member of
// their argument structs.  Workgroup b digests the work items wave_seg[b] .. wave_seg[b+1]-1; a work item is a segment of a
// run (tiles sharing J, K, L, ordered by I >= J) with the directory entries first .. first+count-1.
struct TileDir {
    const double *tiles;
    const int64_t *tile_off;
    const int *tile_I;
    const RunRec *runs;      // segments (runs cut at wave boundaries)
    const int *wave_seg;     // [nwaves+1]
};
static TileDir tile_dir(const mi_ctx *c) { return {c->d_tiles, c->d_tile_off, c->d_tile_I, c->d_segs, c->d_wave_seg}; }

// body(seg, std::bool_constant<nontemporal>) over the work items of blockIdx.x.  PREFIX: the first `n_cached` work items (the
// longest segments) are read with the default cache policy, everything else with nontemporal loads: on a tensor larger than
// the 256 MiB Infinity Cache the nontemporal stream does not evict them, so that share of the tiles is served on-die in every
// SCF cycle after the first instead of from HBM.
template <bool NT, bool PREFIX, class F>
__device__ __forceinline__ void for_work_items(const TileDir &S, const int n_cached, F &&body)
{
    const MI_CONST_AS int *wave_seg = as_const(S.wave_seg);
    const int seg_end = wave_seg[blockIdx.x + 1];
    for (int seg = wave_seg[blockIdx.x]; seg < seg_end; seg++) {
        if (NT && PREFIX && seg < n_cached) body(seg, std::false_type{});
        else body(seg, std::bool_constant<NT>{});
    }
}

// Run header of work item `seg`.  tri: triangular rows in block-diagonal tiles (tile geometry above).
struct RunHead {
    int J, first, count;
    int J0, K0, L0;
    int bk;                  // tiles are padded to 8 j-rows
    bool dkl;                // K == L block diagonal: holds for the whole run or not at all
};
__device__ __forceinline__ RunHead run_head(const TileDir &S, const int seg, const int nao, const bool tri)
{
    const MI_CONST_AS RunRec *rr = as_const(S.runs) + seg;
    const RunRec R{rr->J, rr->K, rr->L, rr->first, rr->count};
    return {R.J, R.first, R.count, R.J * BLK, R.K * BLK, R.L * BLK, min(BLK, nao - R.K * BLK), tri && R.K == R.L};
}

// One tile of a run: directory entry -> geometry
struct TileEntry { int I; int64_t off; };
struct TileHead {
    int I0, bi;
    bool dij;                // I == J block diagonal: only the first tile of a run can lie on it
    int64_t toff;
};
__device__ __forceinline__ TileEntry tile_entry(const TileDir &S, const int tid)
{
    return {as_const(S.tile_I)[tid], as_const(S.tile_off)[tid]};
}
__device__ __forceinline__ TileHead tile_head(const RunHead &R, const TileEntry e, const int nao, const bool tri)
{
    return {e.I * BLK, min(BLK, nao - e.I * BLK), tri && e.I == R.J, e.off};
}
// tile t of the run, whose entry was fetched into `next` one tile ago; the directory entry of tile t+1 is fetched while tile t
// is being digested
__device__ __forceinline__ TileHead tile_step(const TileDir &S, const RunHead &R, const int t, TileEntry &next, const int nao, const bool tri)
{
    const TileHead T = tile_head(R, next, nao, tri);
    if (t + 1 < R.count) next = tile_entry(S, R.first + t + 1);
    return T;
}

struct JkArgs {
    TileDir dir;
    int nruns;               // number of waves
    const double *D; // padded [ldp][ldp]
    double *Jacc, *Kacc;
    int ld, nao;
    int n_cached;            // leading work items read with the default cache policy (kept in the Infinity Cache)
    int tri;                 // triangular rows in block-diagonal tiles (tile geometry)
    size_t pair_stride;      // jk_tiles_pair_kernel: doubles between the two padded densities / accumulator sets
    int pair_sync;           // barrier per tile between the two waves
    int dpp;                 // per-tile reduce-scatters on the DPP path (reduce8_low) instead of ds_bpermute
};

__device__ inline double red_select_xor(double a, double b, bool hi, int mask)
{
    // keep = hi ? b : a ; send = hi ? a : b ; returns keep + partner's send
    double keep = hi ? b : a, send = hi ? a : b;
    return keep + __shfl_xor(send, mask);
}

// reduce-scatter 8 values over the 3 lane bits {m2, m1, m0}; afterwards the lane holds element
// ((lane&m2)?4:0)+((lane&m1)?2:0)+((lane&m0)?1:0)
__device__ inline double reduce8(const double v[8], int lane, int m2, int m1, int m0)
{
    double a[4], b[2];
    bool h2 = lane & m2, h1 = lane & m1, h0 = lane & m0;
#pragma unroll
    for (int t = 0; t < 4; t++) a[t] = red_select_xor(v[t], v[t + 4], h2, m2);
#pragma unroll
    for (int t = 0; t < 2; t++) b[t] = red_select_xor(a[t], a[t + 2], h1, m1);
    return red_select_xor(b[0], b[1], h0, m0);
}

// The same reduce-scatter over the three LOW lane bits (the 8 k-lanes of one i) on the DPP data path instead of the LDS crossbar
// (ds_bpermute: two per double and a ~100-cycle round trip per dependent step, fully exposed at one wave per SIMD).  Step 1 pairs
// lane b with 7 - b (row_half_mirror) instead of b ^ 4: both have opposite bit 2, which is all the first step needs; steps 2 and 3
// (quad_perm) then combine disjoint groups exactly as the xor pattern does, so the lane -> element map is unchanged.
template <int CTRL>
__device__ __forceinline__ double dpp_move(double v)
{
    union { double d; int w[2]; } u, r;
    u.d = v;
    r.w[0] = __builtin_amdgcn_update_dpp(0, u.w[0], CTRL, 0xF, 0xF, false);
    r.w[1] = __builtin_amdgcn_update_dpp(0, u.w[1], CTRL, 0xF, 0xF, false);
    return r.d;
}
__device__ __forceinline__ double reduce8_low(const double v[8], int lane)
{
    constexpr int HALF_MIRROR = 0x141, QP_XOR2 = 0x4E, QP_XOR1 = 0xB1;
    double a[4], b[2];
    const bool h2 = lane & 4, h1 = lane & 2, h0 = lane & 1;
#pragma unroll
    for (int t = 0; t < 4; t++) a[t] = (h2 ? v[t + 4] : v[t]) + dpp_move<HALF_MIRROR>(h2 ? v[t] : v[t + 4]);
#pragma unroll
    for (int t = 0; t < 2; t++) b[t] = (h1 ? a[t + 2] : a[t]) + dpp_move<QP_XOR2>(h1 ? a[t] : a[t + 2]);
    return (h0 ? b[1] : b[0]) + dpp_move<QP_XOR1>(h0 ? b[0] : b[1]);
}

// One 16-byte chunk {T[i,j,k,2lp], T[i,j,k,2lp+1]} of the lane's sub-block.  DIJ / DKL: the tile lies on the I == J / K == L
// block diagonal and stores triangular rows (tile geometry above); for <false,false> this is the plain
// T[(j*4+lp)*bi*bk + i*bk + k] of a full tile.
template <bool DIJ, bool DKL, bool NT>
__device__ __forceinline__ d2_t jk_load_chunk(const d2_t *__restrict__ tile, int j, int lp, int bi, int bk, int i, int k, bool inb)
{
    d2_t x = {0.0, 0.0};
    if (!DIJ && !DKL) {
        if (inb) { const d2_t *q = tile + (i * bk + k) + (size_t)(j * 4 + lp) * (bi * bk); x = NT ? __builtin_nontemporal_load(q) : *q; }
    } else {
        const int i0 = tile_i0(DIJ, j, bi), k0 = tile_k0(DKL, lp, bk);
        const int row = tile_pi(DIJ, j, bi) * tile_qk(DKL, 4, bk) + (bi - i0) * tile_qk(DKL, lp, bk);   // wave-uniform
        if (inb && i >= i0 && k >= k0) { const d2_t *q = tile + row + (i - i0) * (bk - k0) + (k - k0); x = NT ? __builtin_nontemporal_load(q) : *q; }
    }
    return x;
}

// Digestion of one tile by one wave: 32 chunk loads per lane, six contractions per value, per-tile outputs.
// Register budget (J+K, gfx950 ISA): 256 VGPRs + 158 AGPRs, one wave per SIMD; 128 of them are the run-wide K_JL accumulators.
// The compiled tile body is ~1 700 instructions for 384 FMAs: each 16-byte load costs 9 (exec mask for partial blocks, the
// row stride read back from a spilled SGPR, a 64-bit multiply-add), the rest is AGPR traffic, selects and ds_bpermute of the
// reduce-scatters.  A specialisation for full 8x8x8x8 tiles (immediate offsets, no masks) let the scheduler hoist all 32 loads,
// which pushed the kernel to 512 registers and 2.23 ms (from 0.78) -- rejected; scheduling barriers around the tile body did not
// help (498 registers, 2.19 ms).  For the Coulomb-only build the same specialisation is harmless but its gain (0.742 vs 0.754-0.772
// ms on one box, 0.770 vs 0.768-0.772 on another; +8 % on the cache-resident cc-pVDZ tensor) is within box-to-box noise: not kept.
// Any rewrite has to bound the loads in flight by construction.
// Row split (round 3, measured and removed; commit "Experiment: J+K digestion with the j rows of a tile split between two waves"):
// a workgroup of two waves, wave w owning T[i, 4w..4w+3, k, :], 32 K_JL accumulators and partial K_IK / K_IL sums merged through
// LDS (one barrier per tile), fits 256 registers (two waves per SIMD, 132 bytes of scratch) and gives the same J, K, but every
// per-tile fixed cost (density rows, reduce-scatters, directory reads) is paid by both waves: 1.14 ms with the LDS merge, 1.21 ms
// with both waves issuing their own atomics, against 0.86 ms for the one-wave kernel on the same box (benzene/cc-pVTZ).
// KJLT (round 3): K_JL is reduced over the 64 lanes PER TILE (8 DPP reduce-scatters over the k-lanes while the rows stream in,
// one reduce-scatter over the i-lanes, one more 512-byte atomic) instead of living in 64 run-wide accumulators per lane: 128
// registers less, which is what keeps the K-carrying kernel at one wave per SIMD.
template <bool WITH_J, bool WITH_K, bool NT, bool DIJ, bool DKL, bool KJLT = false>
__device__ __forceinline__ void jk_digest_tile(const JkArgs &A, const int lane, const int i, const int k, const RunHead &R, const TileHead &H,
                                               const double (&dKL)[8], const double (&dJK)[8], double (&kjl)[8][8], double (&jkl)[8],
                                               double (&kjk)[8])
{
    const double *__restrict__ D = A.D;
    const MI_CONST_AS double *Du = as_const(A.D);
    const int I0 = H.I0, J0 = R.J0, K0 = R.K0, L0 = R.L0, ld = A.ld, bi = H.bi, bk = R.bk;
    const bool active = (i < bi) && (k < bk);
    const d2_t *__restrict__ T = reinterpret_cast<const d2_t *>(A.dir.tiles + H.toff);
    double dIJ[8], dIL[8];
#pragma unroll
    for (int j = 0; j < 8; j++) dIJ[j] = D[(size_t)(I0 + i) * ld + J0 + j];
#pragma unroll
    for (int l = 0; l < 8; l++) dIL[l] = D[(size_t)(I0 + i) * ld + L0 + l];
    const double dIK = D[(size_t)(I0 + i) * ld + K0 + k];
    double kik = 0.0, jij[8], kil[8], kjl_row[8];
#pragma unroll
    for (int j = 0; j < 8; j++) { jij[j] = 0.0; kil[j] = 0.0; kjl_row[j] = 0.0; }
#pragma unroll
    for (int j = 0; j < 8; j++) {
        double v[8];
#pragma unroll
        for (int lp = 0; lp < 4; lp++) {
            const d2_t x = jk_load_chunk<DIJ, DKL, NT>(T, j, lp, bi, bk, i, k, active);
            v[2 * lp] = x.x; v[2 * lp + 1] = x.y;
        }
        const MI_CONST_AS double *dJL = Du + (size_t)(J0 + j) * ld + L0; // wave-uniform row (SGPRs)
        double pjl[8];
#pragma unroll
        for (int l = 0; l < 8; l++) {
            const double x = v[l];
            if (WITH_K) {
                kik = fma(x, dJL[l], kik);
                kil[l] = fma(x, dJK[j], kil[l]);
                if (KJLT) pjl[l] = x * dIK; else kjl[j][l] = fma(x, dIK, kjl[j][l]);
                kjk[j] = fma(x, dIL[l], kjk[j]);
            }
            if (WITH_J) {
                jij[j] = fma(x, dKL[l], jij[j]);
                jkl[l] = fma(x, dIJ[j], jkl[l]);
            }
        }
        if (WITH_K && KJLT) kjl_row[j] = reduce8_low(pjl, lane);   // sum over the 8 k-lanes of this i; lane holds l = k
    }
    if (WITH_K && KJLT) {
        const double r = reduce8(kjl_row, lane, 32, 16, 8);          // sum over the 8 i-lanes; lane holds j = i
        atomicAdd(&A.Kacc[(size_t)(J0 + i) * ld + L0 + k], r);
    }
    // per-tile outputs: three wave-wide FP64 atomics (1.5 KB added per 32 KB tile; executed at the memory side, not in L2).
    // Their cost, measured by dropping them (wrong J/K, timing only; benzene/cc-pVTZ, same box): J+K launch 0.752 ms without,
    // 0.789-0.84 ms with -- 5-7 % of the launch, about what a scratch buffer of plain stores plus a reduction pass would cost
    // (the same 0.24 GB written, then read), so the atomics stay.
    if (WITH_K) {
        atomicAdd(&A.Kacc[(size_t)(I0 + i) * ld + K0 + k], kik);
        double r = A.dpp ? reduce8_low(kil, lane) : reduce8(kil, lane, 4, 2, 1); // lane holds l = k
        atomicAdd(&A.Kacc[(size_t)(I0 + i) * ld + L0 + k], r);
    }
    if (WITH_J) {
        double r = A.dpp ? reduce8_low(jij, lane) : reduce8(jij, lane, 4, 2, 1); // lane holds j = k
        atomicAdd(&A.Jacc[(size_t)(I0 + i) * ld + J0 + k], r);
    }
}

// Run-wide state of one work item: the run-invariant density rows and the zeroed J_KL / K_JK / K_JL accumulators
__device__ __forceinline__ void jk_run_begin(const double *__restrict__ D, const RunHead &R, const int ld, const int k, double (&dKL)[8],
                                             double (&dJK)[8], double (&kjl)[8][8], double (&jkl)[8], double (&kjk)[8])
{
#pragma unroll
    for (int l = 0; l < 8; l++) dKL[l] = D[(size_t)(R.K0 + k) * ld + R.L0 + l];
#pragma unroll
    for (int j = 0; j < 8; j++) dJK[j] = D[(size_t)(R.J0 + j) * ld + R.K0 + k];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        jkl[j] = 0.0; kjk[j] = 0.0;
#pragma unroll
        for (int l = 0; l < 8; l++) kjl[j][l] = 0.0;
    }
}

// per-run outputs
template <bool WITH_J, bool WITH_K, bool KJLT>
__device__ __forceinline__ void jk_run_end(const JkArgs &A, const RunHead &R, const int lane, const double (&kjl)[8][8],
                                           const double (&jkl)[8], const double (&kjk)[8])
{
    const int i = lane >> 3, k = lane & 7, ld = A.ld;
    if (WITH_J) {
        double r = reduce8(jkl, lane, 32, 16, 8); // lane holds l = i
        atomicAdd(&A.Jacc[(size_t)(R.K0 + k) * ld + R.L0 + i], r);
    }
    if (WITH_K) {
        double r = reduce8(kjk, lane, 32, 16, 8); // lane holds j = i
        atomicAdd(&A.Kacc[(size_t)(R.J0 + i) * ld + R.K0 + k], r);
        // K_JL: 64 values over 64 lanes; first over i-lanes for each l-row... do it as 8 x reduce8 then reduce8
        if (KJLT) return;   // (already added per tile)
        double s[8];
#pragma unroll
        for (int l = 0; l < 8; l++) {
            double col[8];
#pragma unroll
            for (int j = 0; j < 8; j++) col[j] = kjl[j][l];
            s[l] = reduce8(col, lane, 32, 16, 8); // lane holds j = i, summed over i-lanes, for this l
        }
        double r2 = reduce8(s, lane, 4, 2, 1); // lane holds l = k, summed over k-lanes
        atomicAdd(&A.Kacc[(size_t)(R.J0 + i) * ld + R.L0 + k], r2);
    }
}

template <bool WITH_J, bool WITH_K, bool NT, bool PAIR = false, bool KJLT = false>
__device__ __forceinline__ void jk_segment(const JkArgs &A, const int seg)
{
    const int lane = threadIdx.x & 63;
    const int i = lane >> 3, k = lane & 7;
    const RunHead R = run_head(A.dir, seg, A.nao, A.tri);
    double dKL[8], dJK[8], kjl[8][8], jkl[8], kjk[8];
    jk_run_begin(A.D, R, A.ld, k, dKL, dJK, kjl, jkl, kjk);
    TileEntry next = tile_entry(A.dir, R.first);
    auto step = [&](const int t, auto dij, auto dkl) __attribute__((always_inline)) {
        const TileHead H = tile_step(A.dir, R, t, next, A.nao, dij());
        if (PAIR && A.pair_sync) __syncthreads();   // the two waves of a pair stay within one tile of each other: the second reader hits L2
        jk_digest_tile<WITH_J, WITH_K, NT, dij(), dkl(), KJLT>(A, lane, i, k, R, H, dKL, dJK, kjl, jkl, kjk);
    };
    // only the first tile of a run can lie on the I == J diagonal (tiles of a run are ordered by I >= J); K == L holds for
    // the whole run or not at all
    auto tiles = [&](auto dkl) __attribute__((always_inline)) {
        int t = 0;
        if (A.tri && next.I == R.J) step(t++, std::true_type{}, dkl);
        for (; t < R.count; t++) step(t, std::false_type{}, dkl);
    };
    if (R.dkl) tiles(std::true_type{}); else tiles(std::false_type{});
    jk_run_end<WITH_J, WITH_K, KJLT>(A, R, lane, kjl, jkl, kjk);
}

template <bool WITH_J, bool WITH_K, bool NT>
__global__ __launch_bounds__(64) void jk_tiles_kernel(JkArgs A)
{
    for_work_items<NT, true>(A.dir, A.n_cached, [&](const int seg, auto nt) __attribute__((always_inline)) {
        jk_segment<WITH_J, WITH_K, nt()>(A, seg);
    });
}

// J+K with K_JL reduced per tile (KJLT): 128 registers fewer, so two waves fit a SIMD (jk_kjlt option)
template <bool NT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void jk_tiles_kjlt_kernel(JkArgs A)
{
    for_work_items<NT, true>(A.dir, A.n_cached, [&](const int seg, auto nt) __attribute__((always_inline)) {
        jk_segment<true, true, nt(), false, true>(A, seg);
    });
}

// Two densities in ONE pass over the tiles (the spin pair of UHF / UKS).  A single wave cannot hold two sets of
// run-wide accumulators (2 x 64 K_JL + ... : the compiler spills, section 3.1 of DESIGN.md), so a workgroup of TWO waves
// digests one work item: wave 0 with density / accumulators 0, wave 1 with set 1, each with the register budget of the
// single-density kernel, on two SIMDs of one CU.  Both read the same tiles; a barrier per tile keeps them within one tile of
// each other, so the second reader of a 16-byte chunk finds it in L2 (default cache policy: no nontemporal hint here) and
// HBM is read once for both densities.
template <bool WITH_J, bool WITH_K, bool NT>
__global__ __launch_bounds__(128) void jk_tiles_pair_kernel(JkArgs A)
{
    const int wave = threadIdx.x >> 6;
    JkArgs B = A;
    B.D = A.D + wave * A.pair_stride;
    B.Jacc = A.Jacc + wave * A.pair_stride;
    B.Kacc = A.Kacc + wave * A.pair_stride;
    for_work_items<NT, true>(A.dir, A.n_cached, [&](const int seg, auto nt) __attribute__((always_inline)) {
        jk_segment<WITH_J, WITH_K, nt(), true>(B, seg);
    });
}

// Software-pipelined variant for the K-carrying builds (one wave per SIMD, so a wave has to overlap its own
// loads with its own arithmetic): a tile is digested as two halves of 4 j-rows (16 double2 chunks per lane
// each); while half A of tile t is being contracted, half B of tile t is in flight, and while half B is being
// contracted, half A of tile t+1 is in flight.  Same register budget as holding one whole tile.
template <bool DIJ, bool DKL, bool NT>
__device__ __forceinline__ void jk_load_half_t(d2_t (&buf)[16], const d2_t *__restrict__ tile, int bi, int bk, int i, int k, int half)
{
    const bool inb = (i < bi) && (k < bk);
#pragma unroll
    for (int c = 0; c < 16; c++) buf[c] = jk_load_chunk<DIJ, DKL, NT>(tile, half * 4 + (c >> 2), c & 3, bi, bk, i, k, inb);
}
// dij / dkl: wave-uniform diagonal flags of the tile (triangular rows, tile geometry above)
template <bool NT>
__device__ __forceinline__ void jk_load_half(d2_t (&buf)[16], const d2_t *__restrict__ tile, int bi, int bk, int i, int k, bool dij, bool dkl,
                                             int half)
{
    if (dkl) {
        if (dij) jk_load_half_t<true, true, NT>(buf, tile, bi, bk, i, k, half);
        else jk_load_half_t<false, true, NT>(buf, tile, bi, bk, i, k, half);
    } else {
        if (dij) jk_load_half_t<true, false, NT>(buf, tile, bi, bk, i, k, half);
        else jk_load_half_t<false, false, NT>(buf, tile, bi, bk, i, k, half);
    }
}

template <bool WITH_J, bool NT, bool TRI>
__device__ __forceinline__ void jk_pipe_segment(const JkArgs &A, const int seg)
{
    const int lane = threadIdx.x;
    const int i = lane >> 3, k = lane & 7;
    const MI_CONST_AS double *Du = as_const(A.D);
    const double *__restrict__ D = A.D;
    const RunHead R = run_head(A.dir, seg, A.nao, TRI);
    const int J0 = R.J0, K0 = R.K0, L0 = R.L0, ld = A.ld, bk = R.bk;
    double dKL[8], dJK[8], kjl[8][8], jkl[8], kjk[8];
    jk_run_begin(D, R, ld, k, dKL, dJK, kjl, jkl, kjk);

    d2_t bufA[16], bufB[16];
    TileEntry next = tile_entry(A.dir, R.first);
    {
        const TileHead H = tile_head(R, next, A.nao, TRI);
        jk_load_half<NT>(bufA, reinterpret_cast<const d2_t *>(A.dir.tiles + H.toff), H.bi, bk, i, k, H.dij, R.dkl, 0);
    }
    for (int t = 0; t < R.count; t++) {
        const bool more = t + 1 < R.count;
        const TileHead H = tile_step(A.dir, R, t, next, A.nao, TRI);
        const int I0 = H.I0;
        double dIJ[8], dIL[8];
#pragma unroll
        for (int j = 0; j < 8; j++) dIJ[j] = D[(size_t)(I0 + i) * ld + J0 + j];
#pragma unroll
        for (int l = 0; l < 8; l++) dIL[l] = D[(size_t)(I0 + i) * ld + L0 + l];
        const double dIK = D[(size_t)(I0 + i) * ld + K0 + k];
        jk_load_half<NT>(bufB, reinterpret_cast<const d2_t *>(A.dir.tiles + H.toff), H.bi, bk, i, k, H.dij, R.dkl, 1);

        double kik = 0.0, jij[8], kil[8];
#pragma unroll
        for (int j = 0; j < 8; j++) { jij[j] = 0.0; kil[j] = 0.0; }
#pragma unroll
        for (int half = 0; half < 2; half++) {
            d2_t (&buf)[16] = half ? bufB : bufA;
#pragma unroll
            for (int jj = 0; jj < 4; jj++) {
                const int j = half * 4 + jj;
                const MI_CONST_AS double *dJL = Du + (size_t)(J0 + j) * ld + L0;
#pragma unroll
                for (int l = 0; l < 8; l++) {
                    const double x = (l & 1) ? buf[jj * 4 + (l >> 1)].y : buf[jj * 4 + (l >> 1)].x;
                    kik = fma(x, dJL[l], kik);
                    kil[l] = fma(x, dJK[j], kil[l]);
                    kjl[j][l] = fma(x, dIK, kjl[j][l]);
                    kjk[j] = fma(x, dIL[l], kjk[j]);
                    if (WITH_J) {
                        jij[j] = fma(x, dKL[l], jij[j]);
                        jkl[l] = fma(x, dIJ[j], jkl[l]);
                    }
                }
            }
            if (half == 0 && more) {
                const int bin = min(BLK, A.nao - next.I * BLK);
                jk_load_half<NT>(bufA, reinterpret_cast<const d2_t *>(A.dir.tiles + next.off), bin, bk, i, k, false, R.dkl, 0);   // only a run's first tile can have I == J
            }
        }
        atomicAdd(&A.Kacc[(size_t)(I0 + i) * ld + K0 + k], kik);
        {
            double r = reduce8(kil, lane, 4, 2, 1);
            atomicAdd(&A.Kacc[(size_t)(I0 + i) * ld + L0 + k], r);
        }
        if (WITH_J) {
            double r = reduce8(jij, lane, 4, 2, 1);
            atomicAdd(&A.Jacc[(size_t)(I0 + i) * ld + J0 + k], r);
        }
    }
    jk_run_end<WITH_J, true, false>(A, R, lane, kjl, jkl, kjk);
}

// (no default-policy prefix here: every work item is read with the policy of the launch, as mi_jk_describe documents)
template <bool WITH_J, bool NT, bool TRI>
__global__ __launch_bounds__(64) void jk_tiles_pipe_kernel(JkArgs A)
{
    for_work_items<NT, false>(A.dir, 0, [&](const int seg, auto) __attribute__((always_inline)) {
        jk_pipe_segment<WITH_J, NT, TRI>(A, seg);
    });
}

// Dense (nao^4) copy of the resident tiles for post-SCF methods on small molecules (MP2 behind `pyscf.mp`): every stored
// element is un-weighted (tiles hold 1/2 per block coincidence) and written to its eight symmetry images.
__global__ __launch_bounds__(256) void eri_unpack_kernel(const double *tiles, const int64_t *tile_off, const TileInfo *info, int nao,
                                                         int tri, double *out, const int *__restrict__ iperm)
{
    const TileInfo T = info[blockIdx.x];
    const int bi = min(BLK, nao - T.I * BLK), bk = min(BLK, nao - T.K * BLK);
    const int bij = T.I * (T.I + 1) / 2 + T.J, bkl = T.K * (T.K + 1) / 2 + T.L;
    const double *src = tiles + tile_off[blockIdx.x];
    const int ntot = BLK * BLK * bi * bk;
    const size_t n1 = nao, n2 = n1 * nao, n3 = n2 * nao;
    for (int idx = threadIdx.x; idx < ntot; idx += blockDim.x) {
        const int ll = idx & 7, jj = (idx >> 3) & 7, pos = idx >> 6;
        const int ii = pos / bk, kk = pos - ii * bk;
        size_t i = T.I * BLK + ii, j = T.J * BLK + jj, k = T.K * BLK + kk, l = T.L * BLK + ll;
        if (j >= n1 || l >= n1) continue;
        double w;
        const int64_t e = tile_elem(tri != 0, T.I == T.J, T.K == T.L, bij == bkl, bi, bk, ii, jj, kk, ll, &w);
        if (e < 0) continue;                      // the (j,i) / (l,k) partner writes this image
        const double v = src[e] / w;
        i = iperm[i]; j = iperm[j]; k = iperm[k]; l = iperm[l];   // tile order -> the caller's AO order
        out[i * n3 + j * n2 + k * n1 + l] = v; out[j * n3 + i * n2 + k * n1 + l] = v;
        out[i * n3 + j * n2 + l * n1 + k] = v; out[j * n3 + i * n2 + l * n1 + k] = v;
        out[k * n3 + l * n2 + i * n1 + j] = v; out[l * n3 + k * n2 + i * n1 + j] = v;
        out[k * n3 + l * n2 + j * n1 + i] = v; out[l * n3 + k * n2 + j * n1 + i] = v;
    }
}

extern "C" int mi_eri_unpack(mi_ctx *c, double *d_out, void *stream)
{
    if (!c || !d_out) return fail("mi_eri_unpack: null argument");
    if (!c->eri_ready) return fail("mi_eri_unpack: call mi_eri_prepare first");
    if (c->nranks != 1) return fail("mi_eri_unpack: needs the whole (unsharded) tile store");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t n = c->nao;
    HIPCHK(hipMemsetAsync(d_out, 0, sizeof(double) * n * n * n * n, st));   // screened-out tiles stay zero
    if (c->n_tiles == 0) return 0;
    DevBuf<TileInfo> d_info;
    if (d_info.upload(c->tiles)) return -1;
    hipLaunchKernelGGL(eri_unpack_kernel, dim3((unsigned)c->n_tiles), dim3(256), 0, st, c->d_tiles, c->d_tile_off, d_info.get(), c->nao, c->tri, d_out, c->d_iperm);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

// One shell quartet (ish jsh|ksh lsh) read back from the resident tiles: element -> canonical tile position (the inverse of
// put_tile), un-weighted.  NaN where the tile is not resident on this rank (sharded store), 0 where it was screened out.
__global__ void eri_read_quartet_kernel(const double *tiles, const int64_t *tile_off, const int32_t *table, int nao, int ai, int ni,
                                        int aj, int nj, int ak, int nk, int al, int nl, const uint8_t *present, int tri, double *out)
{
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= ni * nj * nk * nl) return;
    int d = idx % nl, c = (idx / nl) % nk, b = (idx / (nl * nk)) % nj, a = idx / (nl * nk * nj);
    int i = ai + a, j = aj + b, k = ak + c, l = al + d;
    if ((i >> 3) < (j >> 3)) { int t = i; i = j; j = t; }
    if ((k >> 3) < (l >> 3)) { int t = k; k = l; l = t; }
    int I = i >> 3, J = j >> 3, K = k >> 3, L = l >> 3;
    int bij = I * (I + 1) / 2 + J, bkl = K * (K + 1) / 2 + L;
    if (bij < bkl) { int t = i; i = k; k = t; t = j; j = l; l = t; t = bij; bij = bkl; bkl = t; I = i >> 3; J = j >> 3; K = k >> 3; L = l >> 3; }
    const size_t slot = (size_t)bij * (bij + 1) / 2 + bkl;
    const int32_t t = table[slot];
    if (t < 0) { out[idx] = (present && present[slot]) ? __builtin_nan("") : 0.0; return; }
    const int bi = min(BLK, nao - I * BLK), bk = min(BLK, nao - K * BLK);
    int ii = i & 7, jj = j & 7, kk = k & 7, ll = l & 7;
    if (tri && I == J && ii < jj) { int t_ = ii; ii = jj; jj = t_; }
    if (tri && K == L && kk < ll) { int t_ = kk; kk = ll; ll = t_; }
    double w;
    const int64_t e = tile_elem(tri != 0, I == J, K == L, bij == bkl, bi, bk, ii, jj, kk, ll, &w);
    out[idx] = tiles[tile_off[t] + e] / w;
}

extern "C" int mi_eri_read_quartet(mi_ctx *c, int ish, int jsh, int ksh, int lsh, double *out)
{
    if (!c || !out) return fail("mi_eri_read_quartet: null argument");
    if (!c->eri_ready) return fail("mi_eri_read_quartet: call mi_eri_prepare first");
    const int sh[4] = {ish, jsh, ksh, lsh};
    for (int s_ : sh) if (s_ < 0 || s_ >= c->nbas) return fail("mi_eri_read_quartet: shell index out of range");
    HIPCHK(hipSetDevice(c->device));
    int ao[4], n[4];
    for (int q = 0; q < 4; q++) { ao[q] = c->shells[sh[q]].ao; n[q] = 2 * c->shells[sh[q]].l + 1; }
    const int tot = n[0] * n[1] * n[2] * n[3];
    DevBuf<double> d_out;
    HIPCHK(d_out.alloc(tot));
    hipLaunchKernelGGL(eri_read_quartet_kernel, dim3((tot + 255) / 256), dim3(256), 0, nullptr, c->d_tiles, c->d_tile_off, c->d_tile_table,
                       c->nao, ao[0], n[0], ao[1], n[1], ao[2], n[2], ao[3], n[3], c->d_tile_present, c->tri, d_out.get());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, d_out, sizeof(double) * tot, hipMemcpyDeviceToHost));
    return 0;
}

// D -> zero-padded [ld][ld] copy, and the J/K accumulators (where given) cleared in the same launch (one kernel instead of three
// per build).  `iperm`: tile AO -> caller AO (the padded copy is in the tile order of the ERI store)
__global__ void pad_density_clear_kernel(const double *D, double *Dp, double *Jacc, double *Kacc, int nao, int ld, const int *__restrict__ iperm)
{
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= ld * ld) return;
    int r = idx / ld, c = idx - r * ld;
    Dp[idx] = (r < nao && c < nao) ? D[(size_t)iperm[r] * nao + iperm[c]] : 0.0;
    if (Jacc) Jacc[idx] = 0.0;
    if (Kacc) Kacc[idx] = 0.0;
}

// `perm`: caller AO -> tile AO (the accumulators are in tile order, J and K leave in the caller's)
__global__ void finalize_jk_kernel(const double *Jacc, const double *Kacc, double *J, double *K, int nao, int ld, const int *__restrict__ perm)
{
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nao * nao) return;
    int r = idx / nao, c = idx - r * nao;
    r = perm[r]; c = perm[c];
    if (J) J[idx] = 2.0 * (Jacc[(size_t)r * ld + c] + Jacc[(size_t)c * ld + r]);
    if (K) K[idx] = Kacc[(size_t)r * ld + c] + Kacc[(size_t)c * ld + r];
}

// tile stream of the J/K, batched J/K and quarter-transformation kernels (option jk_nt): nontemporal loads only when the tensor
// cannot stay in the 256 MiB Infinity Cache between SCF cycles
static bool jk_stream_nt(const mi_ctx *c) { return c->opt_jk_nt != 0 && (c->opt_jk_nt > 1 || c->tile_doubles * 8 > ((int64_t)256 << 20)); }

// Which J/K digestion kernel a build runs, and how: every decision of launch_jk / mi_build_jk lives here, and mi_jk_describe
// reports the same record, so what a caller is told and what is launched cannot drift.
enum JkFamily { JK_PLAIN = 0, JK_KJLT, JK_PIPE, JK_PAIR };
struct JkPlan {
    JkFamily family;
    bool nt;     // nontemporal tile stream (work items below n_jk_cached keep the default policy where the kernel has that split)
    bool dpp;    // per-tile reduce-scatters through DPP moves (the pipeline kernel only has the ds_bpermute form)
};
static JkPlan jk_plan(const mi_ctx *c, bool wj, bool wk, int n_dm)
{
    const int64_t bytes = c->tile_doubles * 8;
    JkPlan P{JK_PLAIN, jk_stream_nt(c), c->opt_jk_dpp != 0};
    // one pass for the pair when it pays: measured -9 % on the 103 GB ibuprofen tensor (UHF cycle 38 -> 34.5 ms), -3 % ... +60 %
    // (erratic) on the 4.9 GB benzene/cc-pVTZ tensor -- so by default only for stores beyond 16 GB (jk_pair = 1: always, 0: never)
    if (n_dm == 2 && (c->opt_jk_pair > 0 || (c->opt_jk_pair < 0 && bytes > ((int64_t)16 << 30)))) { P.family = JK_PAIR; return P; }
    // the half-tile pipeline only exists for full-row tiles: with triangular rows (the default) the plain kernel is the faster
    // one on cache-resident tensors too (benzene/cc-pVDZ J+K 39.8 us vs 41.5 us for full rows + pipeline, 48 us for both)
    const bool pipe = !c->tri && (c->opt_jk_pipe > 0 || (c->opt_jk_pipe < 0 && bytes <= ((int64_t)256 << 20)));
    if (pipe && wk) { P.family = JK_PIPE; P.dpp = false; if (!wj) P.nt = true; }   // (its K-only form is built with the nontemporal stream only)
    else if (wj && wk && c->opt_jk_kjlt) P.family = JK_KJLT;
    return P;
}

// Runtime flags -> template arguments: f(std::bool_constant<flag>...), and f(std::integral_constant<int, W>) for the smallest
// batch width W of 1, 2, 4, 8 that holds n.  A kernel is instantiated where f names it, so f guards the combinations that are
// never launched with `if constexpr`.
template <class F> static void with_flags(F &&f) { f(); }
template <class F, class... B> static void with_flags(F &&f, bool flag, B... rest)
{
    if (flag) with_flags([&](auto... r) { f(std::true_type{}, r...); }, rest...);
    else with_flags([&](auto... r) { f(std::false_type{}, r...); }, rest...);
}
template <class F> static void with_width(int n, F &&f)
{
    if (n <= 1) f(std::integral_constant<int, 1>{});
    else if (n <= 2) f(std::integral_constant<int, 2>{});
    else if (n <= 4) f(std::integral_constant<int, 4>{});
    else f(std::integral_constant<int, 8>{});
}

static int launch_jk_plan(mi_ctx *c, const JkPlan &P, bool wj, bool wk, hipStream_t st)
{
    const bool pair = P.family == JK_PAIR;
    JkArgs A{tile_dir(c), c->n_jk_waves, c->d_Dpad, c->d_Jacc, c->d_Kacc, c->ldp, c->nao,
             c->n_jk_cached, c->tri, (size_t)c->ldp * c->ldp, pair ? 1 : 0, P.dpp ? 1 : 0};
    if (c->n_tiles == 0) return 0;
    if (!wj && !wk) return fail("launch_jk_plan: neither J nor K");
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(A.nruns), dim3(pair ? 128 : 64), 0, st, A); };
    switch (P.family) {
    case JK_PAIR:
        // same cache policy as the single-density kernel: nontemporal stream + default-policy prefix for tensors beyond the
        // Infinity Cache (an all-default-policy stream of 4.9 GB made the launch time erratic: 1.65 ... 2.75 ms)
        with_flags([&](auto J, auto K, auto NT) { if constexpr (J() || K()) launch(jk_tiles_pair_kernel<J(), K(), NT()>); }, wj, wk, P.nt);
        break;
    case JK_PIPE:   // full-row tiles only (jk_plan); the K-only form is built with the nontemporal stream only, whatever P.nt says
        with_flags([&](auto J, auto NT) { launch(jk_tiles_pipe_kernel<J(), J() ? NT() : true, false>); }, wj, P.nt);
        break;
    case JK_KJLT:
        with_flags([&](auto NT) { launch(jk_tiles_kjlt_kernel<NT()>); }, P.nt);
        break;
    case JK_PLAIN:
        with_flags([&](auto J, auto K, auto NT) { if constexpr (J() || K()) launch(jk_tiles_kernel<J(), K(), NT()>); }, wj, wk, P.nt);
        break;
    }
    HIPCHK(hipGetLastError());
    return 0;
}

static int launch_jk(mi_ctx *c, bool wj, bool wk, hipStream_t st) { return launch_jk_plan(c, jk_plan(c, wj, wk, 1), wj, wk, st); }

extern "C" int mi_jk_describe(const mi_ctx *c, int with_j, int with_k, int n_dm, char *buf, size_t len)
{
    if (!c || !buf || len == 0) return fail("mi_jk_describe: null argument");
    if (!c->eri_ready) return fail("mi_jk_describe: call mi_eri_prepare first");
    if ((!with_j && !with_k) || n_dm < 1) return fail("mi_jk_describe: bad argument");
    static const char *const names[] = {"plain", "kjlt", "pipe", "pair"};
    const JkPlan P = jk_plan(c, with_j != 0, with_k != 0, n_dm);
    const int n = snprintf(buf, len, "family=%s nt=%d dpp=%d tri=%d waves=%d segments=%d n_jk_cached=%d", names[P.family], P.nt ? 1 : 0,
                           P.dpp ? 1 : 0, c->tri, c->n_jk_waves, c->n_jk_segs, c->n_jk_cached);
    if (n < 0 || (size_t)n >= len) return fail("mi_jk_describe: buffer of %zu bytes is too small", len);
    return 0;
}

extern "C" int mi_build_jk(mi_ctx *c, const double *d_D, int n_dm, double *d_J, double *d_K, void *stream)
{
    if (!c || !d_D) return fail("mi_build_jk: null argument");
    if (!c->eri_ready) return fail("mi_build_jk: call mi_eri_prepare first");
    if (!d_J && !d_K) return 0;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    size_t nn = (size_t)c->nao * c->nao, pp = (size_t)c->ldp * c->ldp;
    const JkPlan P = jk_plan(c, d_J != nullptr, d_K != nullptr, n_dm);
    const int per = P.family == JK_PAIR ? 2 : 1;   // densities per pass over the tiles (jk_plan: the pair family only for n_dm == 2)
    for (int m0 = 0; m0 < n_dm; m0 += per) {
        const int n = std::min(per, n_dm - m0);
        for (int m = 0; m < n; m++)
            hipLaunchKernelGGL(pad_density_clear_kernel, dim3((unsigned)((pp + 255) / 256)), dim3(256), 0, st, d_D + (m0 + m) * nn, c->d_Dpad + m * pp,
                               d_J ? c->d_Jacc + m * pp : nullptr, d_K ? c->d_Kacc + m * pp : nullptr, c->nao, c->ldp, c->d_iperm);
        if (launch_jk_plan(c, P, d_J != nullptr, d_K != nullptr, st)) return -1;
        for (int m = 0; m < n; m++)
            hipLaunchKernelGGL(finalize_jk_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, st, c->d_Jacc + m * pp, c->d_Kacc + m * pp,
                               d_J ? d_J + (m0 + m) * nn : nullptr, d_K ? d_K + (m0 + m) * nn : nullptr, c->nao, c->ldp, c->d_perm);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

// =================================================================================================
// Batched J/K: n densities per pass over the resident tiles (mi_build_jk_multi; linear response, many trial densities).
//
// A workgroup of two waves digests one work item.  Each tile is read from HBM once, expanded to a full 8x8x8x8 block in LDS
// (triangular rows and ragged edges zero-filled), and contracted against every density of the batch: wave w owns densities
// w, w+2, ...  The six contractions are the three index pairings of the tile read as a 64x64 matrix, each used directly and
// transposed; lane (a, b) produces one output element per pairing and density (a 64-term dot product with the density block,
// whose rows are wave-uniform scalar loads).  Per-tile outputs (J_IJ, K_IK, K_IL) are added with one FP64 atomic per lane and
// density; the run-wide ones (J_KL, K_JL, K_JK) stay in NPW registers each until the run ends.
//
// LDS image: element (i,j,k,l) at JKM_SI*i + JKM_SJ*j + JKM_SK*k + l (4292 doubles).  The strides are purely additive, so every
// read of a pairing is the lane's base plus an immediate offset; with the lane orientations used below the 32 lanes of a
// ds_read_b64 half hit at most two addresses per bank (three pairings conflict-free, three 2-way).
//
// Accumulated contributions.  A stored value x = w (ij|kl) adds x D_jl to K_ik, x D_jk to K_il, x D_ik to K_jl and x D_il to K_jk:
// the four index permutations that keep the bra on the left.  The other four permutations of the quartet, (kl|ij) and its
// swaps, are exactly these four with both sides of the density and of K transposed, so for any D
//   K[D] = Kacc[D] + (Kacc[D^T])^T,
// which is Kacc + Kacc^T for a symmetric and Kacc - Kacc^T for an antisymmetric density.  The set of four is invariant under
// i <-> j and under k <-> l, so the tiles' halved block diagonals (only i >= j stored on I == J, k >= l on K == L, doubled
// weight) give the same Kacc as the full tiles for any density.  J of an antisymmetric density is zero and is not produced.
// =================================================================================================
constexpr int JKM_BATCH = 16;                  // densities per launch: 2 waves x 8
constexpr int JKM_SI = 537, JKM_SJ = 67, JKM_SK = 8;
constexpr int JKM_LDS = 7 * JKM_SI + 7 * JKM_SJ + 7 * JKM_SK + 8;

struct JkmArgs {
    TileDir dir;
    const double *D;           // [n][ld][ld] padded densities in tile order
    double *Jacc, *Kacc;       // [n][ld][ld]
    size_t pp;                 // ld * ld
    int ld, nao, n, jmask;     // jmask bit m: density m is symmetric (J wanted)
    int withk;                 // 0: J only (pure functionals)
    int n_cached, tri;
};

// acc[q] += sum_{c,d} T[base + sc*c + sd*d] * Dq[c*ld + d]  (Dq: the 8x8 density block of density slot q, wave-uniform)
template <int NPW>
__device__ __forceinline__ void jkm_contract(const double *__restrict__ Tl, const int base, const int sc, const int sd,
                                             const MI_CONST_AS double *const (&Dq)[NPW], const int ld, double (&acc)[NPW])
{
#pragma unroll 2
    for (int c = 0; c < 8; c++) {
        double x[8];
#pragma unroll
        for (int d = 0; d < 8; d++) x[d] = Tl[base + sc * c + sd * d];
#pragma unroll
        for (int q = 0; q < NPW; q++) {
            const MI_CONST_AS double *row = Dq[q] + (size_t)c * ld;
#pragma unroll
            for (int d = 0; d < 8; d++) acc[q] = fma(x[d], row[d], acc[q]);
        }
    }
}

// full 8x8x8x8 image of one stored tile in LDS (not-stored and ragged lanes zero), by a workgroup of NTHREADS threads
template <bool NT, int NTHREADS>
__device__ __forceinline__ void load_tile_image(const double *tiles, double *__restrict__ Tl, const int64_t toff, const int bi, const int bk,
                                                const bool dij, const bool dkl)
{
    const d2_t *__restrict__ T = reinterpret_cast<const d2_t *>(tiles + toff);
    // 2048 chunks {T[i,j,k,2m], T[i,j,k,2m+1]} in the store's order (row (j, m), then lanes (i, k)): 16 per thread of 128
    constexpr int NS = 2048 / NTHREADS;
    d2_t v[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) {
        const int c2 = threadIdx.x + NTHREADS * s;
        const int j = c2 >> 8, m = (c2 >> 6) & 3, i = (c2 >> 3) & 7, k = c2 & 7;
        const int ch = (i < bi && k < bk) ? tile_chunk(dij, dkl, bi, bk, i, j, k, m) : -1;
        d2_t x = {0.0, 0.0};
        if (ch >= 0) x = NT ? __builtin_nontemporal_load(T + ch) : T[ch];
        v[s] = x;
    }
#pragma unroll
    for (int s = 0; s < NS; s++) {
        const int c2 = threadIdx.x + NTHREADS * s;
        const int j = c2 >> 8, m = (c2 >> 6) & 3, i = (c2 >> 3) & 7, k = c2 & 7;
        const int a = JKM_SI * i + JKM_SJ * j + JKM_SK * k + 2 * m;
        Tl[a] = v[s].x;
        Tl[a + 1] = v[s].y;
    }
}

template <bool NT, int NPW>
__device__ __forceinline__ void jkm_segment(const JkmArgs &A, double *__restrict__ Tl, const int seg)
{
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int a = lane >> 3, b = lane & 7;
    const RunHead R = run_head(A.dir, seg, A.nao, A.tri);
    const int J0 = R.J0, K0 = R.K0, L0 = R.L0, ld = A.ld;
    // density slots of this wave: m = 2q + wave; slots beyond n repeat density 0 and add nothing
    int mq[NPW];
    bool live[NPW], wantj[NPW];
    bool anyj = false;
#pragma unroll
    for (int q = 0; q < NPW; q++) {
        const int m = 2 * q + wave;
        live[q] = m < A.n;
        mq[q] = live[q] ? m : 0;
        wantj[q] = live[q] && ((A.jmask >> m) & 1);
        anyj |= wantj[q];
    }
    const MI_CONST_AS double *Dc = as_const(A.D);
    double jkl[NPW], kjl[NPW], kjk[NPW];
#pragma unroll
    for (int q = 0; q < NPW; q++) { jkl[q] = 0.0; kjl[q] = 0.0; kjk[q] = 0.0; }
    for (int t = 0; t < R.count; t++) {
        const TileHead H = tile_head(R, tile_entry(A.dir, R.first + t), A.nao, A.tri);
        const int I0 = H.I0;
        __syncthreads();   // the previous tile's image is no longer read
        load_tile_image<NT, 128>(A.dir.tiles, Tl, H.toff, H.bi, R.bk, H.dij, R.dkl);
        __syncthreads();
        const MI_CONST_AS double *Dq[NPW];
        double acc[NPW];
        // J_IJ (lanes i = a, j = b) and J_KL (run-wide; lanes k = a, l = b)
        if (anyj) {
#pragma unroll
            for (int q = 0; q < NPW; q++) { Dq[q] = Dc + mq[q] * A.pp + (size_t)K0 * ld + L0; acc[q] = 0.0; }
            jkm_contract<NPW>(Tl, JKM_SI * a + JKM_SJ * b, JKM_SK, 1, Dq, ld, acc);
#pragma unroll
            for (int q = 0; q < NPW; q++)
                if (wantj[q]) atomicAdd(&A.Jacc[mq[q] * A.pp + (size_t)(I0 + a) * ld + J0 + b], acc[q]);
#pragma unroll
            for (int q = 0; q < NPW; q++) Dq[q] = Dc + mq[q] * A.pp + (size_t)I0 * ld + J0;
            jkm_contract<NPW>(Tl, JKM_SK * a + b, JKM_SI, JKM_SJ, Dq, ld, jkl);
        }
        if (!A.withk) continue;
        // K_IK (lanes k = a, i = b): sum over j, l of T D_JL
#pragma unroll
        for (int q = 0; q < NPW; q++) { Dq[q] = Dc + mq[q] * A.pp + (size_t)J0 * ld + L0; acc[q] = 0.0; }
        jkm_contract<NPW>(Tl, JKM_SK * a + JKM_SI * b, JKM_SJ, 1, Dq, ld, acc);
#pragma unroll
        for (int q = 0; q < NPW; q++)
            if (live[q]) atomicAdd(&A.Kacc[mq[q] * A.pp + (size_t)(I0 + b) * ld + K0 + a], acc[q]);
        // K_IL (lanes i = a, l = b): sum over j, k of T D_JK
#pragma unroll
        for (int q = 0; q < NPW; q++) { Dq[q] = Dc + mq[q] * A.pp + (size_t)J0 * ld + K0; acc[q] = 0.0; }
        jkm_contract<NPW>(Tl, JKM_SI * a + b, JKM_SJ, JKM_SK, Dq, ld, acc);
#pragma unroll
        for (int q = 0; q < NPW; q++)
            if (live[q]) atomicAdd(&A.Kacc[mq[q] * A.pp + (size_t)(I0 + a) * ld + L0 + b], acc[q]);
        // K_JL (run-wide; lanes l = a, j = b): sum over i, k of T D_IK
#pragma unroll
        for (int q = 0; q < NPW; q++) Dq[q] = Dc + mq[q] * A.pp + (size_t)I0 * ld + K0;
        jkm_contract<NPW>(Tl, a + JKM_SJ * b, JKM_SI, JKM_SK, Dq, ld, kjl);
        // K_JK (run-wide; lanes k = a, j = b): sum over i, l of T D_IL
#pragma unroll
        for (int q = 0; q < NPW; q++) Dq[q] = Dc + mq[q] * A.pp + (size_t)I0 * ld + L0;
        jkm_contract<NPW>(Tl, JKM_SK * a + JKM_SJ * b, JKM_SI, 1, Dq, ld, kjk);
    }
#pragma unroll
    for (int q = 0; q < NPW; q++) {
        if (!live[q]) continue;
        const size_t o = mq[q] * A.pp;
        if (wantj[q]) atomicAdd(&A.Jacc[o + (size_t)(K0 + a) * ld + L0 + b], jkl[q]);
        if (!A.withk) continue;
        atomicAdd(&A.Kacc[o + (size_t)(J0 + b) * ld + L0 + a], kjl[q]);
        atomicAdd(&A.Kacc[o + (size_t)(J0 + b) * ld + K0 + a], kjk[q]);
    }
}

template <bool NT, int NPW>
__global__ __launch_bounds__(128) void jk_multi_kernel(JkmArgs A)
{
    __shared__ double Tl[JKM_LDS];
    for_work_items<NT, true>(A.dir, A.n_cached, [&](const int seg, auto nt) __attribute__((always_inline)) {
        jkm_segment<nt(), NPW>(A, Tl, seg);
    });
}

// n densities -> zero-padded [ld][ld] copies in tile order, their accumulators cleared
__global__ void pad_density_multi_kernel(const double *D, double *Dp, double *Jacc, double *Kacc, int n, int nao, int ld,
                                         const int *__restrict__ iperm)
{
    const size_t pp = (size_t)ld * ld;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= pp * n) return;
    const int m = (int)(idx / pp);
    const int64_t e = (int64_t)(idx - (size_t)m * pp);
    const int r = (int)(e / ld), c = (int)(e - (int64_t)r * ld);
    Dp[idx] = (r < nao && c < nao) ? D[(size_t)m * nao * nao + (size_t)iperm[r] * nao + iperm[c]] : 0.0;
    Jacc[idx] = 0.0;
    Kacc[idx] = 0.0;
}

struct JkmSigns { int s[JKM_BATCH]; };
// K = Kacc + s Kacc^T; J = 2 (Jacc + Jacc^T) for s = +1 and 0 for s = -1 (caller's AO order; either output may be NULL)
__global__ void finalize_jk_multi_kernel(const double *Jacc, const double *Kacc, double *J, double *K, int n, int nao, int ld,
                                         const int *__restrict__ perm, JkmSigns sg)
{
    const size_t nn = (size_t)nao * nao, pp = (size_t)ld * ld;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nn * n) return;
    const int m = (int)(idx / nn);
    const int64_t e = (int64_t)(idx - (size_t)m * nn);
    const int r = perm[e / nao], c = perm[e % nao];
    const size_t o = (size_t)m * pp;
    const double s = (double)sg.s[m];
    if (K) K[idx] = Kacc[o + (size_t)r * ld + c] + s * Kacc[o + (size_t)c * ld + r];
    if (J) J[idx] = sg.s[m] > 0 ? 2.0 * (Jacc[o + (size_t)r * ld + c] + Jacc[o + (size_t)c * ld + r]) : 0.0;
}

extern "C" int mi_build_jk_multi(mi_ctx *c, const double *d_D, int n_dm, const int *sym, double *d_J, double *d_K, void *stream)
{
    if (!c || !d_D || !sym || (!d_J && !d_K) || n_dm < 0) return fail("mi_build_jk_multi: null argument");
    if (!c->eri_ready) return fail("mi_build_jk_multi: call mi_eri_prepare first");
    for (int m = 0; m < n_dm; m++)
        if (sym[m] != 1 && sym[m] != -1) return fail("mi_build_jk_multi: sym[m] must be +1 or -1");
    if (n_dm == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t nn = (size_t)c->nao * c->nao, pp = (size_t)c->ldp * c->ldp;
    if (!c->d_mDpad) {
        HIPCHK(dev_malloc(&c->d_mDpad, sizeof(double) * JKM_BATCH * pp));
        HIPCHK(dev_malloc(&c->d_mJacc, sizeof(double) * JKM_BATCH * pp));
        HIPCHK(dev_malloc(&c->d_mKacc, sizeof(double) * JKM_BATCH * pp));
    }
    const int batch = std::max(1, std::min(JKM_BATCH, c->opt_jk_multi_batch));
    const bool nt = jk_stream_nt(c);
    for (int m0 = 0; m0 < n_dm; m0 += batch) {
        const int n = std::min(batch, n_dm - m0);
        JkmSigns sg{};
        int jmask = 0;
        for (int m = 0; m < n; m++) { sg.s[m] = sym[m0 + m]; if (sg.s[m] > 0) jmask |= 1 << m; }
        if (!d_K && !jmask) {   // J only, and every density antisymmetric: J is zero
            HIPCHK(hipMemsetAsync(d_J + m0 * nn, 0, sizeof(double) * nn * n, st));
            continue;
        }
        hipLaunchKernelGGL(pad_density_multi_kernel, dim3((unsigned)((pp * n + 255) / 256)), dim3(256), 0, st, d_D + m0 * nn, c->d_mDpad,
                           c->d_mJacc, c->d_mKacc, n, c->nao, c->ldp, c->d_iperm);
        HIPCHK(hipGetLastError());
        if (c->n_tiles > 0) {
            JkmArgs A{tile_dir(c), c->d_mDpad, c->d_mJacc, c->d_mKacc, pp, c->ldp, c->nao, n, d_J ? jmask : 0, d_K ? 1 : 0, c->n_jk_cached, c->tri};
            with_width((n + 1) / 2, [&](auto NPW) {   // densities per wave
                with_flags([&](auto NT) { hipLaunchKernelGGL((jk_multi_kernel<NT(), NPW()>), dim3(c->n_jk_waves), dim3(128), 0, st, A); }, nt);
            });
            HIPCHK(hipGetLastError());
        }
        hipLaunchKernelGGL(finalize_jk_multi_kernel, dim3((unsigned)((nn * n + 255) / 256)), dim3(256), 0, st, c->d_mJacc, c->d_mKacc,
                           d_J ? d_J + m0 * nn : nullptr, d_K ? d_K + m0 * nn : nullptr, n, c->nao, c->ldp, c->d_perm, sg);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

// =================================================================================================
// Occupied-index quarter transformation of the resident tiles (mi_eri_qtrans; first quarter of the AO -> MO transformation of
// MP2): Y[o][p][q][r] = sum_s C[s][o] (s p|q r) for a batch of n <= QT_BATCH columns of C, one pass over the store per batch.
//
// A stored value x = w (ij|kl) (w: the tile weight of put_tile) adds
//   C_i x to A[j][k][l],   C_j x to A[i][k][l],   C_k x to A[l][i][j],   C_l x to A[k][i][j]
// -- the four images of the quartet that keep (k,l) resp. (i,j) in stored order.  The other four are these with the trailing
// pair swapped, so Y = A + A^T(q <-> r) (finalize kernel; exactly symmetric, a + b == b + a).  The set of eight is invariant under
// i <-> j, k <-> l and (ij) <-> (kl), which is why the halved block diagonals (weight 1/2 per block coincidence, or only i >= j /
// k >= l stored in the triangular layout) give the full sum -- the argument of the batched J/K kernel above.
//
// Work distribution and tile image as in jk_multi_kernel: a workgroup (four waves here) digests one work item, every tile is
// expanded to the full 8x8x8x8 block in LDS (not-stored and ragged lanes zero).  Each of the four contractions has 512 outputs
// per tile and orbital, two per thread; a thread reads its 8 summands from LDS once and uses them for all NB orbitals (the
// coefficients are wave-uniform scalar loads), so LDS traffic per FP64 FMA falls as 1/NB.  A[.][J][K L] is shared by the tiles
// of a run (they differ in I only) and stays in registers until the run ends; the other three are added per tile with FP64
// global atomics into the padded accumulator A[n][ld][ld][ld] (tile AO order).
// =================================================================================================
constexpr int QT_BATCH = 8;                    // orbitals per pass
constexpr int QT_THREADS = 256;

struct QtArgs {
    TileDir dir;
    const double *C;           // [ld][QT_BATCH] coefficient rows in tile order, zero-padded
    double *A;                 // [n][ld][ld][ld]
    size_t p3;                 // ld^3
    int ld, nao, n_cached, tri;
    int n;                     // orbitals of this launch (<= NB of the instantiation; slots beyond it are never written)
};

// acc[o] += sum_c Tl[base + sc * c] * Crow[c][o]  (Crow: 8 coefficient rows of QT_BATCH doubles, wave-uniform)
template <int NB>
__device__ __forceinline__ void qt_contract(const double *__restrict__ Tl, const int base, const int sc,
                                            const MI_CONST_AS double *Crow, double (&acc)[NB])
{
    double x[8];
#pragma unroll
    for (int c = 0; c < 8; c++) x[c] = Tl[base + sc * c];
#pragma unroll
    for (int c = 0; c < 8; c++)
#pragma unroll
        for (int o = 0; o < NB; o++) acc[o] = fma(x[c], Crow[c * QT_BATCH + o], acc[o]);
}

template <bool NT, int NB>
__device__ __forceinline__ void qt_segment(const QtArgs &A, double *__restrict__ Tl, const int seg)
{
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int a = lane >> 3, b = lane & 7;
    const RunHead R = run_head(A.dir, seg, A.nao, A.tri);
    const int J0 = R.J0, K0 = R.K0, L0 = R.L0;
    const size_t ld = A.ld;
    const MI_CONST_AS double *Cc = as_const(A.C);
    double run[2][NB];
#pragma unroll
    for (int s = 0; s < 2; s++)
#pragma unroll
        for (int o = 0; o < NB; o++) run[s][o] = 0.0;
    for (int t = 0; t < R.count; t++) {
        const TileHead H = tile_head(R, tile_entry(A.dir, R.first + t), A.nao, A.tri);
        const int I0 = H.I0;
        __syncthreads();   // the previous tile's image is no longer read
        load_tile_image<NT, QT_THREADS>(A.dir.tiles, Tl, H.toff, H.bi, R.bk, H.dij, R.dkl);
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 2; s++) {
            const int u = wave + 4 * s;      // the output index that is uniform over the wave
            double acc[NB];
            // A[J0+u][K0+a][L0+b] += sum_i C_i T[i,u,a,b]   (run-wide)
            qt_contract<NB>(Tl, JKM_SJ * u + JKM_SK * a + b, JKM_SI, Cc + (size_t)I0 * QT_BATCH, run[s]);
            // A[I0+u][K0+a][L0+b] += sum_j C_j T[u,j,a,b]
#pragma unroll
            for (int o = 0; o < NB; o++) acc[o] = 0.0;
            qt_contract<NB>(Tl, JKM_SI * u + JKM_SK * a + b, JKM_SJ, Cc + (size_t)J0 * QT_BATCH, acc);
#pragma unroll
            for (int o = 0; o < NB; o++)
                if (o < A.n && acc[o] != 0.0) atomicAdd(&A.A[o * A.p3 + ((size_t)(I0 + u) * ld + K0 + a) * ld + L0 + b], acc[o]);
            // A[L0+u][I0+a][J0+b] += sum_k C_k T[a,b,k,u]
#pragma unroll
            for (int o = 0; o < NB; o++) acc[o] = 0.0;
            qt_contract<NB>(Tl, JKM_SI * a + JKM_SJ * b + u, JKM_SK, Cc + (size_t)K0 * QT_BATCH, acc);
#pragma unroll
            for (int o = 0; o < NB; o++)
                if (o < A.n && acc[o] != 0.0) atomicAdd(&A.A[o * A.p3 + ((size_t)(L0 + u) * ld + I0 + a) * ld + J0 + b], acc[o]);
            // A[K0+u][I0+a][J0+b] += sum_l C_l T[a,b,u,l]
#pragma unroll
            for (int o = 0; o < NB; o++) acc[o] = 0.0;
            qt_contract<NB>(Tl, JKM_SI * a + JKM_SJ * b + JKM_SK * u, 1, Cc + (size_t)L0 * QT_BATCH, acc);
#pragma unroll
            for (int o = 0; o < NB; o++)
                if (o < A.n && acc[o] != 0.0) atomicAdd(&A.A[o * A.p3 + ((size_t)(K0 + u) * ld + I0 + a) * ld + J0 + b], acc[o]);
        }
    }
#pragma unroll
    for (int s = 0; s < 2; s++)
#pragma unroll
        for (int o = 0; o < NB; o++)
            if (o < A.n && run[s][o] != 0.0) atomicAdd(&A.A[o * A.p3 + ((size_t)(J0 + wave + 4 * s) * ld + K0 + a) * ld + L0 + b], run[s][o]);
}

template <bool NT, int NB>
__global__ __launch_bounds__(QT_THREADS) void eri_qtrans_kernel(QtArgs A)
{
    __shared__ double Tl[JKM_LDS];
    for_work_items<NT, true>(A.dir, A.n_cached, [&](const int seg, auto nt) __attribute__((always_inline)) {
        qt_segment<nt(), NB>(A, Tl, seg);
    });
}

// Cp[r][o] = C[iperm[r]][o0 + o] for r < nao, o < n; zero elsewhere (tile AO order, QT_BATCH columns)
__global__ void qt_pad_coeff_kernel(const double *C, int ldc, int n, int nao, int ld, double *Cp, const int *__restrict__ iperm)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= ld * QT_BATCH) return;
    const int r = idx / QT_BATCH, o = idx - r * QT_BATCH;
    Cp[idx] = (r < nao && o < n) ? C[(size_t)iperm[r] * ldc + o] : 0.0;
}

// Y[o][p][q][r] = A[o][p'][q'][r'] + A[o][p'][r'][q'] in the caller's AO order (x' = perm[x]), padding dropped
__global__ void qt_finalize_kernel(const double *A, double *Y, int nao, int ld, size_t p3, const int *__restrict__ perm)
{
    const size_t n2 = (size_t)nao * nao;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;     // (p, q, r) of orbital blockIdx.y
    if (idx >= n2 * nao) return;
    const int p = perm[idx / n2], q = perm[(idx / nao) % nao], r = perm[idx % nao];
    const double *Ao = A + blockIdx.y * p3 + (size_t)p * ld * ld;
    Y[blockIdx.y * n2 * nao + idx] = Ao[(size_t)q * ld + r] + Ao[(size_t)r * ld + q];
}

extern "C" int mi_eri_qtrans_batch(void) { return QT_BATCH; }

extern "C" int mi_eri_qtrans(mi_ctx *c, const double *d_C, int nb, int ldc, double *d_Y, void *stream)
{
    if (!c || !d_C || !d_Y || nb < 0 || ldc < nb) return fail("mi_eri_qtrans: bad argument");
    if (!c->eri_ready) return fail("mi_eri_qtrans: call mi_eri_prepare first");
    if (c->nranks != 1) return fail("mi_eri_qtrans: needs the whole (unsharded) tile store");
    if (nb == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t ld = c->ldp, p3 = ld * ld * ld, n3 = (size_t)c->nao * c->nao * c->nao;
    const int nmax = std::min(nb, QT_BATCH);
    DevBuf<double> d_A, d_Cp;
    if (d_A.alloc(p3 * nmax) != hipSuccess) {
        (void)hipGetLastError();
        return fail("mi_eri_qtrans: no device memory for the %.2f GB accumulator", 8e-9 * p3 * nmax);
    }
    if (d_Cp.alloc(ld * QT_BATCH) != hipSuccess) { (void)hipGetLastError(); return fail("mi_eri_qtrans: no device memory"); }
    const bool nt = jk_stream_nt(c);
    int rc = 0;
    for (int m0 = 0; m0 < nb && !rc; m0 += QT_BATCH) {
        const int n = std::min(QT_BATCH, nb - m0);
        hipLaunchKernelGGL(qt_pad_coeff_kernel, dim3((unsigned)((ld * QT_BATCH + 255) / 256)), dim3(256), 0, st, d_C + m0, ldc, n, c->nao,
                           (int)ld, d_Cp.get(), c->d_iperm);
        if (hipMemsetAsync(d_A, 0, sizeof(double) * p3 * n, st) != hipSuccess) { rc = fail("mi_eri_qtrans: memset failed"); break; }
        if (c->n_tiles > 0) {
            QtArgs A{tile_dir(c), d_Cp, d_A, p3, (int)ld, c->nao, c->n_jk_cached, c->tri, n};
            with_width(n, [&](auto NB) {
                with_flags([&](auto NT) { hipLaunchKernelGGL((eri_qtrans_kernel<NT(), NB()>), dim3(c->n_jk_waves), dim3(QT_THREADS), 0, st, A); }, nt);
            });
        }
        hipLaunchKernelGGL(qt_finalize_kernel, dim3((unsigned)((n3 + 255) / 256), (unsigned)n), dim3(256), 0, st, d_A.get(), d_Y + (size_t)m0 * n3,
                           c->nao, (int)ld, p3, c->d_perm);
        if (hipGetLastError() != hipSuccess) rc = fail("mi_eri_qtrans: kernel launch failed");
    }
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = fail("mi_eri_qtrans: %s", hipGetErrorString(hipGetLastError()));
    return rc;
}

// =================================================================================================
// Active-pair Coulomb operators of the resident tiles (mi_eri_active_j; the two-electron input of a CASSCF macro iteration):
//   Jp[vw][p][q] = sum_rs (pq|rs) Ca[r][v] Ca[s][w],   v >= w packed as v (v + 1) / 2 + w,
// for up to AJ_WIDTH pairs per pass over the store.  This is the J half of jk_multi_kernel for the symmetric densities
// D_vw[r][s] = (Ca[r][v] Ca[s][w] + Ca[s][v] Ca[r][w]) / 2 (same weights, same accumulate-then-symmetrise rule, see there), with two
// differences: the densities are never in memory, and the contractions run on the FP64 matrix unit.
//
// A tile read as the 64x64 matrix T[(ij)][(kl)] gives   Jacc[.][I J] += T D_KL   (per tile)   and   Jacc[.][K L] += T^T D_IJ
// (shared by the tiles of a run: kept in the MFMA accumulators until the run ends), each a 64x64 by 64xN product with one
// column per pair.  v_mfma_f64_16x16x4_f64 takes the 4x16 slice D[(kl) = 4 s + (lane >> 4)][pair = lane & 15] as ONE double per
// lane, so a lane builds its density elements from the coefficient rows of its own pair (v, w) in registers -- lane-varying
// operands are what the matrix unit wants and what the VALU form (wave-uniform operands from scalar loads, as qt_contract)
// cannot take without first writing the densities to memory.  Wave `wave` of the four owns the 16 output rows
// 16 wave .. 16 wave + 15 of both products; the A operand is one ds_read_b64 of the tile image per lane and k-step, shared by
// the NB column blocks.  Result registers (guide: col = lane & 15, row = (lane >> 4) + 4 reg) go out with one FP64 atomic each
// into the accumulator Jacc[ld][ld][AJ_WIDTH] (pair index fastest: the 16 lanes of a row group write 128 contiguous bytes).
// =================================================================================================
constexpr int AJ_WIDTH = 32;                   // pairs per pass: 2 column blocks of the 16-wide MFMA
constexpr int AJ_MAXCAS = 16;
constexpr int AJ_THREADS = 256;
typedef double d4_t __attribute__((ext_vector_type(4)));

struct AjArgs {
    TileDir dir;
    const double *C;           // two [ld][QT_BATCH] panels (orbitals 0..7, 8..15) in tile order, zero-padded
    double *Jacc;              // [ld][ld][AJ_WIDTH]
    int ld, nao, n_cached, tri;
    int m0, n;                 // first pair and number of pairs of this pass (n <= 16 NB)
};

template <bool NT, int NB>
__device__ __forceinline__ void aj_segment(const AjArgs &A, double *__restrict__ Tl, const int seg)
{
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int col = lane & 15, g = lane >> 4;
    const RunHead R = run_head(A.dir, seg, A.nao, A.tri);
    const int J0 = R.J0, K0 = R.K0, L0 = R.L0;
    const size_t ld = A.ld;
    const size_t panel = ld * QT_BATCH;
    // this lane's pair per column block: offsets of its two orbitals' columns in the coefficient panels; `h` = 1/2 (live) or 0
    int ov[NB], ow[NB];
    double h[NB];
#pragma unroll
    for (int nb = 0; nb < NB; nb++) {
        const int ml = 16 * nb + col, m = A.m0 + ml;
        int v = 0;
        while ((v + 1) * (v + 2) / 2 <= m && v < AJ_MAXCAS - 1) v++;
        const int w = min(m - v * (v + 1) / 2, v);
        ov[nb] = (v >> 3) * (int)panel + (v & 7);
        ow[nb] = (w >> 3) * (int)panel + (w & 7);
        h[nb] = ml < A.n ? 0.5 : 0.0;
    }
    const double *__restrict__ Cp = A.C;
    // D_KL in B-operand form, fixed over the run: k-step s holds (k, l) = (s >> 1, 4 (s & 1) + g)
    double dkl[NB][16];
#pragma unroll
    for (int nb = 0; nb < NB; nb++) {
        double lv[2], lw[2];
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const size_t r = (size_t)(L0 + 4 * e + g) * QT_BATCH;
            lv[e] = h[nb] * Cp[r + ov[nb]];
            lw[e] = h[nb] * Cp[r + ow[nb]];
        }
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const size_t r = (size_t)(K0 + k) * QT_BATCH;
            const double kv = Cp[r + ov[nb]], kw = Cp[r + ow[nb]];
#pragma unroll
            for (int e = 0; e < 2; e++) dkl[nb][2 * k + e] = fma(kv, lw[e], kw * lv[e]);
        }
    }
    // the J rows of D_IJ are fixed over the run as well: j = 4 e + g
    double jv[NB][2], jw[NB][2];
#pragma unroll
    for (int nb = 0; nb < NB; nb++)
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const size_t r = (size_t)(J0 + 4 * e + g) * QT_BATCH;
            jv[nb][e] = h[nb] * Cp[r + ov[nb]];
            jw[nb][e] = h[nb] * Cp[r + ow[nb]];
        }
    d4_t run[NB];
#pragma unroll
    for (int nb = 0; nb < NB; nb++) run[nb] = d4_t{0.0, 0.0, 0.0, 0.0};
    // A-operand bases: row (lane & 15) of this wave's 16, i.e. (2 wave + (col >> 3), col & 7) of the leading index pair
    const int hi = 2 * wave + (col >> 3), lo = col & 7;
    const int base_ij = JKM_SI * hi + JKM_SJ * lo + g;           // + JKM_SK * k + 4 e   : T[(i j)][(k l)]
    const int base_kl = JKM_SK * hi + lo + JKM_SJ * g;           // + JKM_SI * i + 4 JKM_SJ e : T[(i j)][(k l)] read by (k l)
    for (int t = 0; t < R.count; t++) {
        const TileHead H = tile_head(R, tile_entry(A.dir, R.first + t), A.nao, A.tri);
        const int I0 = H.I0;
        __syncthreads();   // the previous tile's image is no longer read
        load_tile_image<NT, AJ_THREADS>(A.dir.tiles, Tl, H.toff, H.bi, R.bk, H.dij, R.dkl);
        // D_IJ of this tile while the image settles: k-step s holds (i, j) = (s >> 1, 4 (s & 1) + g)
        double dij[NB][16];
#pragma unroll
        for (int nb = 0; nb < NB; nb++)
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const size_t r = (size_t)(I0 + i) * QT_BATCH;
                const double iv = Cp[r + ov[nb]], iw = Cp[r + ow[nb]];
#pragma unroll
                for (int e = 0; e < 2; e++) dij[nb][2 * i + e] = fma(iv, jw[nb][e], iw * jv[nb][e]);
            }
        __syncthreads();
        d4_t acc[NB];
#pragma unroll
        for (int nb = 0; nb < NB; nb++) acc[nb] = d4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 16; s++) {
            const double x = Tl[base_ij + JKM_SK * (s >> 1) + 4 * (s & 1)];
            const double y = Tl[base_kl + JKM_SI * (s >> 1) + 4 * JKM_SJ * (s & 1)];
#pragma unroll
            for (int nb = 0; nb < NB; nb++) {
                acc[nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(x, dkl[nb][s], acc[nb], 0, 0, 0);
                run[nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(y, dij[nb][s], run[nb], 0, 0, 0);
            }
        }
        // result register q: row g + 4 q of the wave's 16 = (i, j) = (2 wave + (q >> 1), g + 4 (q & 1))
#pragma unroll
        for (int nb = 0; nb < NB; nb++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const double val = acc[nb][q];
                if (16 * nb + col < A.n && val != 0.0)
                    atomicAdd(&A.Jacc[((size_t)(I0 + 2 * wave + (q >> 1)) * ld + J0 + g + 4 * (q & 1)) * AJ_WIDTH + 16 * nb + col], val);
            }
    }
#pragma unroll
    for (int nb = 0; nb < NB; nb++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const double val = run[nb][q];
            if (16 * nb + col < A.n && val != 0.0)
                atomicAdd(&A.Jacc[((size_t)(K0 + 2 * wave + (q >> 1)) * ld + L0 + g + 4 * (q & 1)) * AJ_WIDTH + 16 * nb + col], val);
        }
}

template <bool NT, int NB>
__global__ __launch_bounds__(AJ_THREADS) void eri_active_j_kernel(AjArgs A)
{
    __shared__ double Tl[JKM_LDS];
    for_work_items<NT, true>(A.dir, A.n_cached, [&](const int seg, auto nt) __attribute__((always_inline)) {
        aj_segment<nt(), NB>(A, Tl, seg);
    });
}

// Jp[m0 + m][p][q] = 2 (Jacc[p'][q'][m] + Jacc[q'][p'][m]) in the caller's AO order (x' = perm[x]): exactly symmetric
__global__ void aj_finalize_kernel(const double *Jacc, double *Jp, int n, int nao, int ld, const int *__restrict__ perm)
{
    const size_t nn = (size_t)nao * nao;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nn * n) return;
    const int m = (int)(idx % n);
    const size_t e = idx / n;
    const size_t r = perm[e / nao], c = perm[e % nao];
    Jp[(size_t)m * nn + e] = 2.0 * (Jacc[(r * ld + c) * AJ_WIDTH + m] + Jacc[(c * ld + r) * AJ_WIDTH + m]);
}

extern "C" int mi_eri_active_j_width(void) { return AJ_WIDTH; }

extern "C" int mi_eri_active_j(mi_ctx *c, const double *d_Ca, int ncas, int ldc, double *d_Jp, void *stream)
{
    if (!c || !d_Ca || !d_Jp || ncas < 1 || ncas > AJ_MAXCAS || ldc < ncas) return fail("mi_eri_active_j: bad argument (1 <= ncas <= 16, ldc >= ncas)");
    if (!c->eri_ready) return fail("mi_eri_active_j: call mi_eri_prepare first");
    if (c->nranks != 1) return fail("mi_eri_active_j: needs the whole (unsharded) tile store");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t ld = c->ldp, nn = (size_t)c->nao * c->nao;
    const int npair = ncas * (ncas + 1) / 2;
    DevBuf<double> d_acc, d_Cp;
    if (d_acc.alloc(ld * ld * AJ_WIDTH) != hipSuccess || d_Cp.alloc(2 * ld * QT_BATCH) != hipSuccess) {
        (void)hipGetLastError();
        return fail("mi_eri_active_j: no device memory");
    }
    for (int o0 = 0; o0 < AJ_MAXCAS; o0 += QT_BATCH)   // orbitals beyond ncas: zero columns
        hipLaunchKernelGGL(qt_pad_coeff_kernel, dim3((unsigned)((ld * QT_BATCH + 255) / 256)), dim3(256), 0, st, d_Ca + std::min(o0, ncas - 1), ldc,
                           std::max(0, std::min(QT_BATCH, ncas - o0)), c->nao, (int)ld, d_Cp.get() + (size_t)(o0 / QT_BATCH) * ld * QT_BATCH, c->d_iperm);
    const bool nt = jk_stream_nt(c);
    int rc = 0;
    for (int m0 = 0; m0 < npair && !rc; m0 += AJ_WIDTH) {
        const int n = std::min(AJ_WIDTH, npair - m0);
        if (hipMemsetAsync(d_acc, 0, sizeof(double) * ld * ld * AJ_WIDTH, st) != hipSuccess) { rc = fail("mi_eri_active_j: memset failed"); break; }
        if (c->n_tiles > 0) {
            AjArgs A{tile_dir(c), d_Cp, d_acc, (int)ld, c->nao, c->n_jk_cached, c->tri, m0, n};
            with_flags([&](auto NT, auto WIDE) {
                hipLaunchKernelGGL((eri_active_j_kernel<NT(), WIDE() ? 2 : 1>), dim3(c->n_jk_waves), dim3(AJ_THREADS), 0, st, A);
            }, nt, n > 16);
        }
        hipLaunchKernelGGL(aj_finalize_kernel, dim3((unsigned)((nn * n + 255) / 256)), dim3(256), 0, st, d_acc.get(), d_Jp + (size_t)m0 * nn, n,
                           c->nao, (int)ld, c->d_perm);
        if (hipGetLastError() != hipSuccess) rc = fail("mi_eri_active_j: kernel launch failed");
    }
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = fail("mi_eri_active_j: %s", hipGetErrorString(hipGetLastError()));
    return rc;
}

extern "C" int mi_time_jk_variant(mi_ctx *c, const double *d_D, int with_j, int with_k, int reps, double *ms, void *stream)
{
    if (!c || !d_D || !ms || reps < 1 || (!with_j && !with_k)) return fail("mi_time_jk_variant: bad argument");
    if (!c->eri_ready) return fail("mi_time_jk_variant: call mi_eri_prepare first");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    size_t pp = (size_t)c->ldp * c->ldp;
    hipLaunchKernelGGL(pad_density_clear_kernel, dim3((unsigned)((pp + 255) / 256)), dim3(256), 0, st, d_D, c->d_Dpad, c->d_Jacc, c->d_Kacc,
                       c->nao, c->ldp, c->d_iperm);
    struct Event {   // released on every return
        hipEvent_t e = nullptr;
        ~Event() { if (e) hipEventDestroy(e); }
    } e0, e1;
    HIPCHK(hipEventCreate(&e0.e));
    HIPCHK(hipEventCreate(&e1.e));
    if (launch_jk(c, with_j != 0, with_k != 0, st)) return -1; // warm
    HIPCHK(hipEventRecord(e0.e, st));
    for (int r = 0; r < reps; r++)
        if (launch_jk(c, with_j != 0, with_k != 0, st)) return -1;
    HIPCHK(hipEventRecord(e1.e, st));
    HIPCHK(hipEventSynchronize(e1.e));
    float t = 0;
    HIPCHK(hipEventElapsedTime(&t, e0.e, e1.e));
    *ms = (double)t / reps;
    return 0;
}

extern "C" int mi_time_jk_kernel(mi_ctx *c, const double *d_D, int reps, double *ms, void *stream)
{
    return mi_time_jk_variant(c, d_D, 1, 1, reps, ms, stream);
}

// =================================================================================================
// DIIS helpers
// =================================================================================================
__global__ void diis_errvec_kernel(const double *sdf, double *err, int n)
{
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * n) return;
    int r = idx / n, c = idx - r * n;
    err[idx] = sdf[(size_t)c * n + r] - sdf[idx];
}

extern "C" int mi_diis_errvec(mi_ctx *c, const double *d_SDF, double *d_err, void *stream)
{
    if (!c) return fail("null context");
    int n = c->nao;
    hipLaunchKernelGGL(diis_errvec_kernel, dim3((n * n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_SDF, d_err, n);
    HIPCHK(hipGetLastError());
    return 0;
}

struct CoefPack { double c[16]; };
__global__ void diis_combine_kernel(const double *hist, CoefPack cf, int n, size_t nn, double *out)
{
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nn) return;
    double s = 0.0;
    for (int i = 0; i < n; i++) s = fma(cf.c[i], hist[(size_t)i * nn + idx], s);
    out[idx] = s;
}

extern "C" int mi_diis_combine(mi_ctx *c, const double *d_hist, const double *coef, int n, double *d_out, void *stream)
{
    if (!c || n < 1 || n > 16) return fail("mi_diis_combine: bad argument");
    CoefPack cf{};
    for (int i = 0; i < n; i++) cf.c[i] = coef[i];
    size_t nn = (size_t)c->nao * c->nao;
    hipLaunchKernelGGL(diis_combine_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_hist, cf, n, nn, d_out);
    HIPCHK(hipGetLastError());
    return 0;
}

// Gram row of the DIIS error vectors: out[i * DIIS_NS + s] = partial dot product <hist_e[i], e> over slice s of the
// vector (grid = n x DIIS_NS blocks; the caller adds the DIIS_NS partials in index order: deterministic, and 16x the
// parallelism of one block per history vector).
#define DIIS_NS 16
__global__ __launch_bounds__(256) void diis_dots_kernel(const double *hist, const double *e, size_t nn, double *out)
{
    __shared__ double sh[4];
    const double *h = hist + (size_t)blockIdx.x * nn;
    const size_t per = (nn + DIIS_NS - 1) / DIIS_NS, lo = per * blockIdx.y, hi = lo + per < nn ? lo + per : nn;
    double p[4] = {0, 0, 0, 0};
    size_t i = lo + threadIdx.x;
    for (; i + 3 * 256 < hi; i += 4 * 256) {
#pragma unroll
        for (int u = 0; u < 4; u++) p[u] = fma(h[i + u * 256], e[i + u * 256], p[u]);
    }
    for (; i < hi; i += 256) p[0] = fma(h[i], e[i], p[0]);
    double s = (p[0] + p[1]) + (p[2] + p[3]);
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x * DIIS_NS + blockIdx.y] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

extern "C" int mi_diis_dots_dev_n(mi_ctx *c, const double *d_hist_e, const double *d_e, int n, int64_t len, double *d_out, void *stream)
{
    if (!c || n < 1 || n > 64 || len < 1 || !d_out) return fail("mi_diis_dots_dev_n: bad argument");
    hipLaunchKernelGGL(diis_dots_kernel, dim3(n, DIIS_NS), dim3(256), 0, (hipStream_t)stream, d_hist_e, d_e, (size_t)len, d_out);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int mi_diis_dots_dev(mi_ctx *c, const double *d_hist_e, const double *d_e, int n, double *d_out, void *stream)
{
    if (!c) return fail("mi_diis_dots_dev: bad argument");
    return mi_diis_dots_dev_n(c, d_hist_e, d_e, n, (int64_t)c->nao * c->nao, d_out, stream);
}

// CDIIS without the host: one small workgroup adds the Gram-row partials of the newest error vector in index order, updates the
// device-resident B matrix (row and column `slot` of [space][space]) and solves Pulay's (m+1) x (m+1) system
//   [0 1^T; 1 B] [lambda; c] = [1; 0]
// by Gaussian elimination with partial pivoting on the rows (the largest |entry| of the column, the first row on ties; row
// updates are fused multiply-adds), then back substitution; c[0..m) goes to d_coef for diis_combine_dev_kernel.  There is no
// rank guard: the only fallback, c = e_slot (no extrapolation), is taken when a pivot is exactly zero or not finite or a
// back-substituted value is not finite -- error vectors exactly zero, a history holding the same pair twice to the bit, a NaN
// or Inf among the partials.  A merely ill-conditioned history is solved as it stands, backward stably (the
// contract B1-B5 and what tests/test_gpu_diis_chain.py measured).  Same instruction sequence on every rank of a sharded run,
// so the coefficients are bit-identical there.
#define DIIS_MAXM 16
// value of `x` on lane `l` (wave-uniform l) through v_readlane: no LDS crossbar trip, unlike __shfl with a runtime lane
__device__ __forceinline__ double lane_bcast(double x, int l)
{
    const int ls = __builtin_amdgcn_readfirstlane(l);
    const long long b = __double_as_longlong(x);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(b & 0xffffffffll), ls);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), ls);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
// One wave, the augmented system [n][n + 1] in LDS, every loop rolled: 5 KB of code.  Lane r owns row r, the pivot is found with a
// wave reduction, the pivot row is read as LDS broadcasts, back substitution is column oriented.  Three implementations measured
// the same 14 us per launch (4.8 us of it the floor of any kernel here): rows in LDS with lane 0 scanning for the pivot; a fully
// unrolled register / v_readlane version (41 KB of code); this one.  What is left is a chain of ~60 dependent LDS / cross-lane
// round trips on one wave plus two dependent global round trips (partials in, coefficients out).
__global__ __launch_bounds__(64) void diis_solve_kernel(const double *__restrict__ part, int m, int slot, int space, double *B, double *__restrict__ coef)
{
    __shared__ double A[DIIS_MAXM + 1][DIIS_MAXM + 3];   // column n holds the right-hand side
    __shared__ double X[DIIS_MAXM + 1];
    const int t = threadIdx.x;
    const int n = m + 1;
    // older Gram entries of this lane's row and the partial sums of the newest row: all requested before anything waits
    double bold[DIIS_MAXM];
#pragma unroll
    for (int j = 0; j < DIIS_MAXM; j++) bold[j] = (t >= 1 && t <= m && j < m) ? B[(t - 1) * space + j] : 0.0;
    double dot = 0.0;                         // lane i < m: <e_i, e_slot>
    if (t < m) {
        double pq[DIIS_NS];
#pragma unroll
        for (int q = 0; q < DIIS_NS; q++) pq[q] = part[t * DIIS_NS + q];
#pragma unroll
        for (int q = 0; q < DIIS_NS; q++) dot += pq[q];
        B[slot * space + t] = dot;
        B[t * space + slot] = dot;
        X[t] = dot;                           // staged for the other lanes (row / column `slot` of the system)
    }
    __syncthreads();
    if (t < n) {
#pragma unroll
        for (int j = 0; j <= DIIS_MAXM; j++) {
            double v = 0.0;
            if (j < n) {
                if (t == 0) v = (j == 0) ? 0.0 : 1.0;
                else if (j == 0) v = 1.0;
                else if (t - 1 == slot) v = X[j - 1];
                else if (j - 1 == slot) v = X[t - 1];
                else v = bold[j - 1];
            }
            A[t][j] = v;
        }
        A[t][n] = (t == 0) ? 1.0 : 0.0;
    }
    __syncthreads();
    bool ok = true;
    for (int k = 0; k < n && ok; k++) {
        // pivot: largest |A[r][k]|, r = k .. n-1, the first one on ties (LAPACK's idamax)
        double val = (t >= k && t < n) ? fabs(A[t][k]) : -1.0;
        int p = t;
        for (int o = 32; o > 0; o >>= 1) {
            const double v2 = __shfl_xor(val, o);
            const int p2 = __shfl_xor(p, o);
            if (v2 > val || (v2 == val && p2 < p)) { val = v2; p = p2; }
        }
        if (!(val > 0.0) || !isfinite(val)) { ok = false; break; }        // wave-uniform
        if (p != k && t <= n) { const double x = A[k][t]; A[k][t] = A[p][t]; A[p][t] = x; }   // lane t swaps column t
        __syncthreads();
        if (t > k && t < n) {
            const double f = A[t][k] / A[k][k];
            for (int j = k; j <= n; j++) A[t][j] = fma(-f, A[k][j], A[t][j]);
        }
        __syncthreads();
    }
    if (ok) {
        for (int i = n - 1; i >= 0; i--) {
            if (t == i) X[i] = A[i][n] / A[i][i];
            __syncthreads();
            const double xi = X[i];
            if (!isfinite(xi)) ok = false;                                   // wave-uniform (every lane reads the same value)
            if (t < i) A[t][n] = fma(-A[t][i], xi, A[t][n]);
            __syncthreads();
        }
    }
    if (t >= 1 && t <= m) coef[t - 1] = ok ? X[t] : ((t - 1) == slot ? 1.0 : 0.0);
}

extern "C" int mi_diis_solve(mi_ctx *c, const double *d_part, int m, int slot, int space, double *d_B, double *d_coef, void *stream)
{
    if (!c || !d_part || !d_B || !d_coef || m < 1 || m > DIIS_MAXM || space < m || slot < 0 || slot >= m) return fail("mi_diis_solve: bad argument");
    hipLaunchKernelGGL(diis_solve_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, d_part, m, slot, space, d_B, d_coef);
    HIPCHK(hipGetLastError());
    return 0;
}

__global__ void diis_combine_dev_kernel(const double *hist, const double *coef, int n, size_t nn, double *out)
{
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nn) return;
    const MI_CONST_AS double *cf = as_const(coef);
    double s = 0.0;
    for (int i = 0; i < n; i++) s = fma(cf[i], hist[(size_t)i * nn + idx], s);
    out[idx] = s;
}

extern "C" int mi_diis_combine_dev_n(mi_ctx *c, const double *d_hist, const double *d_coef, int n, int64_t len, double *d_out, void *stream)
{
    if (!c || !d_hist || !d_coef || !d_out || n < 1 || n > DIIS_MAXM || len < 1) return fail("mi_diis_combine_dev_n: bad argument");
    hipLaunchKernelGGL(diis_combine_dev_kernel, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_hist, d_coef, n, (size_t)len, d_out);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int mi_diis_combine_dev(mi_ctx *c, const double *d_hist, const double *d_coef, int n, double *d_out, void *stream)
{
    if (!c) return fail("mi_diis_combine_dev: bad argument");
    return mi_diis_combine_dev_n(c, d_hist, d_coef, n, (int64_t)c->nao * c->nao, d_out, stream);
}

extern "C" int mi_diis_dots(mi_ctx *c, const double *d_hist_e, const double *d_e, int n, double *out, void *stream)
{
    if (!c || n < 1 || n > 64) return fail("mi_diis_dots: bad argument");
    size_t nn = (size_t)c->nao * c->nao;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(diis_dots_kernel, dim3(n, DIIS_NS), dim3(256), 0, st, d_hist_e, d_e, nn, c->d_red);
    HIPCHK(hipGetLastError());
    double part[64 * DIIS_NS];
    HIPCHK(hipMemcpyAsync(part, c->d_red, sizeof(double) * n * DIIS_NS, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int i = 0; i < n; i++) {
        double s = 0.0;
        for (int q = 0; q < DIIS_NS; q++) s += part[i * DIIS_NS + q];
        out[i] = s;
    }
    return 0;
}

// =================================================================================================
// DFT: Becke weights, AO values on the grid, density, XC functionals, weighted AOs (rows a7-a9)
// =================================================================================================
#define MAXATM_LDS 1024

struct BeckeArgs {
    const double *coords; // [ng][3]
    const int32_t *atom_of;
    const double *vol;
    const double *atom_xyz; // [natm][3]
    const double *adj;      // [natm][natm] Treutler adjustment a_ij
    int natm;
    int64_t ng;
    double *w;
};

// One step f(x) = (3 - x^2) x / 2 of the Becke polynomial, written as x + x (1 - x^2) / 2 with 1 - x^2 from one fma (the product is
// not rounded).  From anywhere within 2^-27 of +-1 this lands on +-1 exactly, so a point on a nucleus or on an interatomic axis
// (mu = +-1 up to the rounding of rsqrt) gets cell functions of exactly 0 and 1.  (3.0 - x * x) * x * 0.5 does not: at
// x = 1 - 2^-53 the difference 3 - x^2 rounds to 2, the step returns x, and the cell function stays at 2^-54.
__device__ __forceinline__ double becke_step(double x) { return fma(0.5 * x, fma(-x, x, 1.0), x); }

// One thread per grid point.  P_i = prod_{j != i} s(mu_ij), 3x iterated Becke polynomial, with
// mu' = mu + a_ij (1 - mu^2); w = vol * P_owner / sum_i P_i.
__global__ __launch_bounds__(256) void becke_weights_kernel(BeckeArgs A)
{
    extern __shared__ double sh[]; // atom coordinates
    for (int i = threadIdx.x; i < A.natm * 3; i += blockDim.x) sh[i] = A.atom_xyz[i];
    __syncthreads();
    int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= A.ng) return;
    const double x = A.coords[3 * g], y = A.coords[3 * g + 1], z = A.coords[3 * g + 2];
    const int own = A.atom_of[g];
    double psum = 0.0, pown = 0.0;
    for (int i = 0; i < A.natm; i++) {
        double dxi = x - sh[3 * i], dyi = y - sh[3 * i + 1], dzi = z - sh[3 * i + 2];
        double ri = sqrt(dxi * dxi + dyi * dyi + dzi * dzi);
        double p = 1.0;
        for (int j = 0; j < A.natm; j++) {
            if (j == i) continue;
            double dxj = x - sh[3 * j], dyj = y - sh[3 * j + 1], dzj = z - sh[3 * j + 2];
            double rj = sqrt(dxj * dxj + dyj * dyj + dzj * dzj);
            double ax = sh[3 * i] - sh[3 * j], ay = sh[3 * i + 1] - sh[3 * j + 1], az = sh[3 * i + 2] - sh[3 * j + 2];
            double mu = (ri - rj) * rsqrt(ax * ax + ay * ay + az * az);
            mu = mu + A.adj[i * A.natm + j] * (1.0 - mu * mu);
            mu = becke_step(becke_step(becke_step(mu)));
            p *= 0.5 * (1.0 - mu);
        }
        psum += p;
        if (i == own) pown = p;
    }
    A.w[g] = A.vol[g] * pown / psum;
}

extern "C" int mi_grid_becke(mi_ctx *c, const double *d_coords, const int32_t *d_atom_of, const double *d_vol, int64_t ng,
                             const double *d_adjust, double *d_weights, void *stream)
{
    if (!c) return fail("mi_grid_becke: null context");
    if (ng < 0) return fail("mi_grid_becke: negative number of grid points");
    if (ng == 0) return 0;   // nothing to write (a zero-sized grid would be a launch error)
    if (!d_coords || !d_atom_of || !d_vol || !d_adjust || !d_weights) return fail("mi_grid_becke: null argument");
    if (c->natm > MAXATM_LDS) return fail("mi_grid_becke: too many atoms");
    HIPCHK(hipSetDevice(c->device));
    std::vector<double> xyz(c->natm * 3);
    for (int i = 0; i < c->natm; i++)
        for (int d = 0; d < 3; d++) xyz[3 * i + d] = c->env[c->atm[i * ATM_SLOTS + 1] + d];
    DevBuf<double> d_xyz;
    HIPCHK(d_xyz.alloc(xyz.size()));
    HIPCHK(hipMemcpy(d_xyz, xyz.data(), sizeof(double) * xyz.size(), hipMemcpyHostToDevice));
    BeckeArgs A{d_coords, d_atom_of, d_vol, d_xyz, d_adjust, c->natm, ng, d_weights};
    hipLaunchKernelGGL(becke_weights_kernel, dim3((unsigned)((ng + 255) / 256)), dim3(256), sizeof(double) * 3 * c->natm,
                       (hipStream_t)stream, A);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

// ---- grid-weight response: out_C += sum_g e_g vol_g d[P_o / sum_B P_B](r_g; R) / dR_C, the point moving with its parent o ----
struct BeckeGradArgs {
    const double *coords; // [ng][3] of this chunk of points
    const int32_t *atom_of;
    const double *vol;
    const double *e;        // unweighted energy density per point
    const double *atom_xyz; // [natm][3]
    const double *adj;      // [natm][natm]
    int natm;
    int64_t ng;
    double *cell;           // [natm][ldc]: the cell functions P_i of every point of the chunk (each lane reads back its own column)
    int64_t ldc;
    double *part;           // [waves][natm][3]: one private row per wave, summed in a fixed order by becke_grad_reduce_kernel
};

// One lane per grid point.  With s_ij = s(nu_ij), s_ji = 1 - s_ij (mu, a and the polynomial are odd under i <-> j) and
// q_i = e vol (delta_io - P_o/Z) P_i / Z, the pair {C, j} moves atom C by
//     (q_C / s_Cj - q_j / s_jC) s'(nu_Cj) (1 - 2 a_Cj mu_Cj) dmu_Cj/dR_C,     dmu_Cj/dR_C = -(u_C + mu_Cj e_Cj) / R_Cj,
// u_C the unit vector from atom C to the point (zero for a point on the nucleus) and e_Cj the one from j to C.  The point's
// own derivative is minus the sum of the two atom derivatives of every pair, so the parent atom gets -sum_C (all of the above).
// Pass 1 is the pair loop of becke_weights_kernel (same arithmetic, so the same P_i to the bit) and leaves P_i in `cell`;
// pass 2 loops over the target atom C with three register accumulators and one wave reduction per C; pass 3 books the
// accumulated point derivative to the parent atoms present in the wave.
// q_i / s_ij stands for q_i's product without the factor s_ij and is formed only where s_ij > 0 (then s_ij >= 2^-54 and the
// quotient is exact to rounding).  1 - f3 rounds to exactly zero within 7e-3 of nu = 1; there P_i is exactly zero too, and the
// pair contributes exactly zero, never 0/0.  What that drops is s' times the other factors, below 6e-14 per unit of e vol --
// the size of the rounding of 1 - f3 itself, which the weights carry as well.
__global__ __launch_bounds__(256) void becke_grad_kernel(BeckeGradArgs A)
{
    extern __shared__ double sh[]; // atom coordinates
    for (int i = threadIdx.x; i < A.natm * 3; i += blockDim.x) sh[i] = A.atom_xyz[i];
    __syncthreads();
    const int natm = A.natm;
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = g < A.ng;
    const int64_t gl = live ? g : A.ng - 1;   // lanes past the end stay in the wave reductions with a zero coefficient
    const double x = A.coords[3 * gl], y = A.coords[3 * gl + 1], z = A.coords[3 * gl + 2];
    const int own = A.atom_of[gl];
    const double ev = live ? A.e[gl] * A.vol[gl] : 0.0;
    double *cell = A.cell + gl;
    double psum = 0.0, pown = 0.0;
    for (int i = 0; i < natm; i++) {
        double dxi = x - sh[3 * i], dyi = y - sh[3 * i + 1], dzi = z - sh[3 * i + 2];
        double ri = sqrt(dxi * dxi + dyi * dyi + dzi * dzi);
        double p = 1.0;
        for (int j = 0; j < natm; j++) {
            if (j == i) continue;
            double dxj = x - sh[3 * j], dyj = y - sh[3 * j + 1], dzj = z - sh[3 * j + 2];
            double rj = sqrt(dxj * dxj + dyj * dyj + dzj * dzj);
            double ax = sh[3 * i] - sh[3 * j], ay = sh[3 * i + 1] - sh[3 * j + 1], az = sh[3 * i + 2] - sh[3 * j + 2];
            double mu = (ri - rj) * rsqrt(ax * ax + ay * ay + az * az);
            mu = mu + A.adj[i * natm + j] * (1.0 - mu * mu);
            mu = becke_step(becke_step(becke_step(mu)));
            p *= 0.5 * (1.0 - mu);
        }
        psum += p;
        if (i == own) pown = p;
        if (live) cell[(int64_t)i * A.ldc] = p;
    }
    const double zinv = 1.0 / psum;
    const double qo = ev * zinv, qz = ev * pown * zinv * zinv;   // q_i = (delta_io qo - qz) P_i
    double *row = A.part + ((size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * (size_t)(natm * 3);
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int C = 0; C < natm; C++) {
        const double cx = sh[3 * C], cy = sh[3 * C + 1], cz = sh[3 * C + 2];
        const double dxc = x - cx, dyc = y - cy, dzc = z - cz;
        const double rc = sqrt(dxc * dxc + dyc * dyc + dzc * dzc);
        const double rci = rc > 0.0 ? 1.0 / rc : 0.0;
        const double ucx = dxc * rci, ucy = dyc * rci, ucz = dzc * rci;
        const double qC = ((C == own ? qo : 0.0) - qz) * (live ? cell[(int64_t)C * A.ldc] : 0.0);
        double gx = 0.0, gy = 0.0, gz = 0.0;
        for (int j = 0; j < natm; j++) {
            if (j == C) continue;
            const double dxj = x - sh[3 * j], dyj = y - sh[3 * j + 1], dzj = z - sh[3 * j + 2];
            const double rj = sqrt(dxj * dxj + dyj * dyj + dzj * dzj);
            const double ex = cx - sh[3 * j], ey = cy - sh[3 * j + 1], ez = cz - sh[3 * j + 2];
            const double rinv = rsqrt(ex * ex + ey * ey + ez * ez);
            const double mu = (rc - rj) * rinv;
            const double a = A.adj[C * natm + j];
            const double nu = mu + a * (1.0 - mu * mu);
            const double f1 = becke_step(nu), f2 = becke_step(f1), f3 = becke_step(f2);
            const double sp = -1.6875 * (1.0 - f2 * f2) * (1.0 - f1 * f1) * (1.0 - nu * nu);   // s'(nu) = -1/2 (3/2)^3 prod (1 - f_k^2)
            const double sCj = 0.5 * (1.0 - f3), sjC = 0.5 * (1.0 + f3);
            const double qj = ((j == own ? qo : 0.0) - qz) * (live ? cell[(int64_t)j * A.ldc] : 0.0);
            const double t = (sCj > 0.0 ? qC / sCj : 0.0) - (sjC > 0.0 ? qj / sjC : 0.0);
            const double k = -t * sp * (1.0 - 2.0 * a * mu) * rinv;
            const double me = mu * rinv;
            gx += k * (ucx + me * ex);
            gy += k * (ucy + me * ey);
            gz += k * (ucz + me * ez);
        }
        sx += gx; sy += gy; sz += gz;
        for (int o = 32; o > 0; o >>= 1) { gx += __shfl_xor(gx, o); gy += __shfl_xor(gy, o); gz += __shfl_xor(gz, o); }
        if (lane == 0) { row[3 * C] = gx; row[3 * C + 1] = gy; row[3 * C + 2] = gz; }
    }
    unsigned long long pending = __ballot(live);
    while (pending) {   // wave-uniform: one round per parent atom present in the wave
        const int oc = __shfl(own, __ffsll((long long)pending) - 1);
        const bool mine = live && own == oc;
        double gx = mine ? sx : 0.0, gy = mine ? sy : 0.0, gz = mine ? sz : 0.0;
        for (int o = 32; o > 0; o >>= 1) { gx += __shfl_xor(gx, o); gy += __shfl_xor(gy, o); gz += __shfl_xor(gz, o); }
        if (lane == 0 && oc >= 0 && oc < natm) { row[3 * oc] -= gx; row[3 * oc + 1] -= gy; row[3 * oc + 2] -= gz; }   // the lane that wrote the row
        pending &= ~__ballot(mine);
    }
}

// out[c] += sum_w part[w][c]: one workgroup per component, a strided partial sum per thread and an LDS tree -- the order
// depends on the number of waves only, so the result is reproducible to the bit.
__global__ __launch_bounds__(256) void becke_grad_reduce_kernel(const double *part, int64_t nw, int n3, double *out)
{
    __shared__ double red[256];
    const int c = blockIdx.x;
    double s = 0.0;
    for (int64_t w = threadIdx.x; w < nw; w += 256) s += part[(size_t)w * n3 + c];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[c] += red[0];
}

#define BECKE_GRAD_CELL_DOUBLES ((int64_t)1 << 25)   // cap of the cell-function workspace (256 MB): larger grids go in chunks of points

extern "C" int mi_grid_becke_grad(mi_ctx *c, const double *d_coords, const int32_t *d_atom_of, const double *d_vol, const double *d_e,
                                  int64_t ng, const double *d_adjust, double *d_out, void *stream)
{
    if (!c || !d_coords || !d_atom_of || !d_vol || !d_e || !d_adjust || !d_out) return fail("mi_grid_becke_grad: null argument");
    if (c->natm > MAXATM_LDS) return fail("mi_grid_becke_grad: too many atoms");
    if (ng < 0) return fail("mi_grid_becke_grad: negative number of grid points");
    if (ng == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    const int natm = c->natm;
    std::vector<double> xyz(natm * 3);
    for (int i = 0; i < natm; i++)
        for (int d = 0; d < 3; d++) xyz[3 * i + d] = c->env[c->atm[i * ATM_SLOTS + 1] + d];
    DevBuf<double> d_xyz, d_cell, d_part;
    HIPCHK(d_xyz.alloc(xyz.size()));
    HIPCHK(hipMemcpy(d_xyz, xyz.data(), sizeof(double) * xyz.size(), hipMemcpyHostToDevice));
    const int64_t chunk = std::min<int64_t>((ng + 255) / 256 * 256, std::max<int64_t>(256, BECKE_GRAD_CELL_DOUBLES / natm / 256 * 256));
    const int64_t waves = chunk / 64;
    HIPCHK(d_cell.alloc((size_t)natm * chunk));
    HIPCHK(d_part.alloc((size_t)waves * natm * 3));
    for (int64_t p0 = 0; p0 < ng; p0 += chunk) {
        const int64_t n = std::min(chunk, ng - p0);
        const int64_t nblk = (n + 255) / 256;
        BeckeGradArgs A{d_coords + 3 * p0, d_atom_of + p0, d_vol + p0, d_e + p0, d_xyz, d_adjust, natm, n, d_cell, chunk, d_part};
        hipLaunchKernelGGL(becke_grad_kernel, dim3((unsigned)nblk), dim3(256), sizeof(double) * 3 * natm, st, A);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(becke_grad_reduce_kernel, dim3(natm * 3), dim3(256), 0, st, d_part.get(), nblk * 4, natm * 3, d_out);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(st));   // the workspaces are freed on return
    return 0;
}

struct AoArgs : BasisDev {
    int deriv;
    const double *coords; // [ng][3]
    int64_t ng;
    double *ao;           // [1 | 4 | 10][nao][ng]: value; +gradient; +second derivatives xx,xy,xz,yy,yz,zz
};

// One thread per grid point, loop over shells (wave-uniform shell data -> scalar loads); stores are
// coalesced along the grid index.
// One shell at one grid point with compile-time angular momentum and derivative order: every loop bound is a constant, so
// the spherical accumulators (up to 10 x 7 doubles for an f shell with second derivatives) live in registers instead of
// the 528 B of scratch per thread the runtime-l version needed.
template <int L, int DERIV>
__device__ __forceinline__ void eval_ao_shell(const AoArgs &A, const int32_t *b, int ish, int64_t g, double x, double y, double z)
{
    constexpr int ns = 2 * L + 1;
    const int np = b[2];
    const double r2 = x * x + y * y + z * z;
    double rad = 0.0, drad = 0.0, d2rad = 0.0;
    for (int p = 0; p < np; p++) {
        double a = A.env[b[5] + p];
        double e = A.env[b[6] + p] * exp(-a * r2);
        rad += e;
        if (DERIV >= 1) drad -= 2.0 * a * e;
        if (DERIV >= 2) d2rad += 4.0 * a * a * e;
    }
    const double *c2s = A.c2s + A.c2s_off[L];
    double s[ns], s1[3][ns], s2[6][ns];
#pragma unroll
    for (int m = 0; m < ns; m++) {
        s[m] = 0.0;
#pragma unroll
        for (int q = 0; q < 3; q++) s1[q][m] = 0.0;
#pragma unroll
        for (int q = 0; q < 6; q++) s2[q][m] = 0.0;
    }
    double px[L + 1], py[L + 1], pz[L + 1];
    px[0] = py[0] = pz[0] = 1.0;
#pragma unroll
    for (int k = 1; k <= L; k++) { px[k] = px[k - 1] * x; py[k] = py[k - 1] * y; pz[k] = pz[k - 1] * z; }
    int k = 0;
#pragma unroll
    for (int lx = L; lx >= 0; lx--)
#pragma unroll
        for (int ly = L - lx; ly >= 0; ly--, k++) {
            const int lz = L - lx - ly;
            const double v = px[lx] * py[ly] * pz[lz];
            double dx = 0.0, dy = 0.0, dz = 0.0, h2[6] = {0, 0, 0, 0, 0, 0};
            if (DERIV >= 1) {
                dx = lx ? lx * px[lx > 0 ? lx - 1 : 0] * py[ly] * pz[lz] : 0.0;
                dy = ly ? ly * px[lx] * py[ly > 0 ? ly - 1 : 0] * pz[lz] : 0.0;
                dz = lz ? lz * px[lx] * py[ly] * pz[lz > 0 ? lz - 1 : 0] : 0.0;
            }
            if (DERIV >= 2) {
                h2[0] = lx > 1 ? lx * (lx - 1) * px[lx > 1 ? lx - 2 : 0] * py[ly] * pz[lz] : 0.0;
                h2[1] = (lx && ly) ? lx * ly * px[lx > 0 ? lx - 1 : 0] * py[ly > 0 ? ly - 1 : 0] * pz[lz] : 0.0;
                h2[2] = (lx && lz) ? lx * lz * px[lx > 0 ? lx - 1 : 0] * py[ly] * pz[lz > 0 ? lz - 1 : 0] : 0.0;
                h2[3] = ly > 1 ? ly * (ly - 1) * px[lx] * py[ly > 1 ? ly - 2 : 0] * pz[lz] : 0.0;
                h2[4] = (ly && lz) ? ly * lz * px[lx] * py[ly > 0 ? ly - 1 : 0] * pz[lz > 0 ? lz - 1 : 0] : 0.0;
                h2[5] = lz > 1 ? lz * (lz - 1) * px[lx] * py[ly] * pz[lz > 1 ? lz - 2 : 0] : 0.0;
            }
#pragma unroll
            for (int m = 0; m < ns; m++) {
                const double cc = c2s[k * ns + m];
                s[m] += cc * v;
                if (DERIV >= 1) { s1[0][m] += cc * dx; s1[1][m] += cc * dy; s1[2][m] += cc * dz; }
                if (DERIV >= 2) {
#pragma unroll
                    for (int q = 0; q < 6; q++) s2[q][m] += cc * h2[q];
                }
            }
        }
    const int ao0 = A.shell_ao[ish];
    const size_t comp = (size_t)A.nao * A.ng;
    const double xyz[3] = {x, y, z};
#pragma unroll
    for (int m = 0; m < ns; m++) {
        const size_t o = (size_t)(ao0 + m) * A.ng + g;
        A.ao[o] = rad * s[m];
        if (DERIV >= 1) {
#pragma unroll
            for (int q = 0; q < 3; q++) A.ao[(1 + q) * comp + o] = drad * xyz[q] * s[m] + rad * s1[q][m];
        }
        if (DERIV >= 2) {
            int q = 0;
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = i; j < 3; j++, q++)
                    A.ao[(4 + q) * comp + o] = d2rad * xyz[i] * xyz[j] * s[m] + (i == j ? drad * s[m] : 0.0) +
                                               drad * (xyz[i] * s1[j][m] + xyz[j] * s1[i][m]) + rad * s2[q][m];
        }
    }
}

template <int DERIV>
__global__ __launch_bounds__(256) void eval_ao_kernel(AoArgs A)
{
    int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= A.ng) return;
    const double gx = A.coords[3 * g], gy = A.coords[3 * g + 1], gz = A.coords[3 * g + 2];
    for (int ish = 0; ish < A.nbas; ish++) {
        const int32_t *b = A.bas + ish * BAS_SLOTS;
        const double *R = A.env + A.atm[b[0] * ATM_SLOTS + 1];
        const double x = gx - R[0], y = gy - R[1], z = gz - R[2];
        switch (b[1]) {   // wave-uniform
        case 0: eval_ao_shell<0, DERIV>(A, b, ish, g, x, y, z); break;
        case 1: eval_ao_shell<1, DERIV>(A, b, ish, g, x, y, z); break;
        case 2: eval_ao_shell<2, DERIV>(A, b, ish, g, x, y, z); break;
        default: eval_ao_shell<3, DERIV>(A, b, ish, g, x, y, z); break;
        }
    }
}

extern "C" int mi_eval_ao(mi_ctx *c, const double *d_coords, int64_t ng, int deriv, double *d_ao, void *stream)
{
    if (!c) return fail("mi_eval_ao: null context");
    if (check_orbital_lmax(c, "mi_eval_ao")) return -1;
    if (ng < 0) return fail("mi_eval_ao: negative number of grid points");
    if (deriv < 0 || deriv > 2) return fail("mi_eval_ao: deriv must be 0, 1 or 2 (got %d)", deriv);
    if (ng == 0) return 0;   // nothing to write (a zero-sized grid would be a launch error)
    if (!d_coords || !d_ao) return fail("mi_eval_ao: null argument");
    HIPCHK(hipSetDevice(c->device));
    AoArgs A{basis_dev(c)};
    A.deriv = deriv; A.coords = d_coords; A.ng = ng; A.ao = d_ao;
    const dim3 grid((unsigned)((ng + 255) / 256)), block(256);
    if (deriv == 0) hipLaunchKernelGGL(eval_ao_kernel<0>, grid, block, 0, (hipStream_t)stream, A);
    else if (deriv == 1) hipLaunchKernelGGL(eval_ao_kernel<1>, grid, block, 0, (hipStream_t)stream, A);
    else hipLaunchKernelGGL(eval_ao_kernel<2>, grid, block, 0, (hipStream_t)stream, A);
    HIPCHK(hipGetLastError());
    return 0;
}

// rho[0][g] = sum_mu ao0*C ; rho[1..3][g] = 2 sum_mu ao_k*C   with C = D @ ao0
__global__ __launch_bounds__(256) void xc_rho_kernel(const double *ao, const double *C, int nao, int64_t ng, int deriv, double *rho)
{
    int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ng) return;
    const size_t comp = (size_t)nao * ng;
    double r0 = 0, r1 = 0, r2 = 0, r3 = 0;
    for (int m = 0; m < nao; m++) {
        size_t o = (size_t)m * ng + g;
        double cv = C[o];
        r0 = fma(ao[o], cv, r0);
        if (deriv) {
            r1 = fma(ao[comp + o], cv, r1);
            r2 = fma(ao[2 * comp + o], cv, r2);
            r3 = fma(ao[3 * comp + o], cv, r3);
        }
    }
    rho[g] = r0;
    if (deriv) { rho[ng + g] = 2 * r1; rho[2 * ng + g] = 2 * r2; rho[3 * ng + g] = 2 * r3; }
}

extern "C" int mi_xc_rho(mi_ctx *c, const double *d_ao, const double *d_C, int64_t ng, int deriv, double *d_rho, void *stream)
{
    if (!c) return fail("mi_xc_rho: null context");
    if (ng < 0) return fail("mi_xc_rho: negative number of grid points");
    if (ng == 0) return 0;   // nothing to write (a zero-sized grid would be a launch error)
    if (!d_ao || !d_C || !d_rho) return fail("mi_xc_rho: null argument");
    hipLaunchKernelGGL(xc_rho_kernel, dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_ao, d_C, c->nao, ng, deriv, d_rho);
    HIPCHK(hipGetLastError());
    return 0;
}

// The same densities from OCCUPIED-ORBITAL values on the grid (numint.eval_rho2 [MEM]): psi[(1|4)][nocc][ng] = Z^T ao with
// D = Z Z^T (rank nocc << nao), rho = sum_i psi_i^2, grad rho = 2 sum_i psi_i grad psi_i, tau = 1/2 sum_i |grad psi_i|^2.
// nao/nocc times fewer bytes and flops than the D.ao route when the density is a projector (every SCF cycle).
__global__ __launch_bounds__(256) void xc_rho_mo_kernel(const double *psi, int nocc, int64_t ng, int deriv, double *rho, double *tau)
{
    int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ng) return;
    const size_t comp = (size_t)nocc * ng;
    double r0 = 0, r1 = 0, r2 = 0, r3 = 0, tk = 0;
    for (int m = 0; m < nocc; m++) {
        size_t o = (size_t)m * ng + g;
        const double p0 = psi[o];
        r0 = fma(p0, p0, r0);
        if (deriv) {
            const double px = psi[comp + o], py = psi[2 * comp + o], pz = psi[3 * comp + o];
            r1 = fma(px, p0, r1); r2 = fma(py, p0, r2); r3 = fma(pz, p0, r3);
            tk = fma(px, px, fma(py, py, fma(pz, pz, tk)));
        }
    }
    rho[g] = r0;
    if (deriv) { rho[ng + g] = 2 * r1; rho[2 * ng + g] = 2 * r2; rho[3 * ng + g] = 2 * r3; }
    if (tau) tau[g] = 0.5 * tk;
}

// Warm start of the low-rank (Nystrom) factor of the projector, one launch instead of ~14 elementwise / reduction launches:
//   good  = every element of Zt [nocc][n] is finite and the Cholesky factorisation reported info == 0
//   scale = 1 / sqrt(max(sum_c Zt[0][c]^2, 1e-300))
//   G[r][c] = good ? 0.05 G0[r][c] + scale Zt[c][r] : G0[r][c]           (G, G0: [n][nocc])
// Every workgroup recomputes the two reductions in the same fixed order (the factor is a few hundred KB in L2) and writes its
// share of G: deterministic, no second launch.  (dft.RKS._lowrank_factor; PySCF has no counterpart -- it takes the occupied
// orbitals from the diagonalisation [MEM: numint.eval_rho2].)
__global__ __launch_bounds__(256) void nystrom_warm_kernel(const double *__restrict__ Zt, const int *__restrict__ info,
                                                           const double *__restrict__ G0, double *__restrict__ G, int nocc, int n)
{
    __shared__ double sh_s[4];
    __shared__ int sh_f[4];
    const int t = threadIdx.x;
    const size_t tot = (size_t)nocc * n;
    int finite = 1;
    double s = 0.0;
    for (size_t idx = t; idx < tot; idx += 256) {
        const double v = Zt[idx];
        finite &= (int)isfinite(v);
        if (idx < (size_t)n) s = fma(v, v, s);     // row 0
    }
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o); finite &= __shfl_xor(finite, o); }
    if ((t & 63) == 0) { sh_s[t >> 6] = s; sh_f[t >> 6] = finite; }
    __syncthreads();
    const double ssum = (sh_s[0] + sh_s[1]) + (sh_s[2] + sh_s[3]);
    const bool good = (sh_f[0] & sh_f[1] & sh_f[2] & sh_f[3]) && info[0] == 0;
    const double scale = 1.0 / sqrt(fmax(ssum, 1e-300));
    for (size_t idx = (size_t)blockIdx.x * 256 + t; idx < tot; idx += (size_t)gridDim.x * 256) {
        const int r = (int)(idx / nocc), c = (int)(idx - (size_t)r * nocc);
        G[idx] = good ? fma(scale, Zt[(size_t)c * n + r], 0.05 * G0[idx]) : G0[idx];
    }
}

// Quadrature sums of one grid block in ONE launch: tail[q] += sum_g w[g] v_q[g] for q < nv (N_elec, E_xc; the two spin counts
// and E_xc for UKS) -- replaces nv rocBLAS dots (two launches each) and nv adds.  Deterministic: every workgroup reduces a
// contiguous chunk in a fixed tree and stores its partials; the workgroup that arrives LAST (ticket from an agent-scope atomic,
// fences around it) adds all partials in index order.  scratch: [XT_MAXWG][3] doubles + the ticket counter, owned by the context.
#define XT_MAXWG 256
struct XcTailArgs { const double *w; const double *v[3]; int nv; int64_t ng; double *tail; double *scratch; unsigned *ticket; };
__global__ __launch_bounds__(256) void xc_tail_kernel(XcTailArgs A)
{
    __shared__ double sh[3][4];
    __shared__ int last;
    const int t = threadIdx.x, nwg = gridDim.x;
    const int64_t per = (A.ng + nwg - 1) / nwg, lo = per * blockIdx.x, hi = min(A.ng, lo + per);
    double s[3] = {0.0, 0.0, 0.0};
    for (int64_t g = lo + t; g < hi; g += 256) {
        const double wg = A.w[g];
#pragma unroll
        for (int q = 0; q < 3; q++) if (q < A.nv) s[q] = fma(wg, A.v[q][g], s[q]);
    }
#pragma unroll
    for (int q = 0; q < 3; q++) {
        for (int o = 32; o > 0; o >>= 1) s[q] += __shfl_xor(s[q], o);
        if ((t & 63) == 0) sh[q][t >> 6] = s[q];
    }
    __syncthreads();
    if (t == 0) {
        for (int q = 0; q < A.nv; q++) A.scratch[blockIdx.x * 3 + q] = (sh[q][0] + sh[q][1]) + (sh[q][2] + sh[q][3]);
        __threadfence();                                             // partials visible before the ticket
        const unsigned k = __hip_atomic_fetch_add(A.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        last = (k == (unsigned)nwg - 1u);
        if (last) {
            __threadfence();
            for (int q = 0; q < A.nv; q++) {
                double tot = 0.0;
                for (int b = 0; b < nwg; b++) tot += __hip_atomic_load(A.scratch + b * 3 + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                A.tail[q] += tot;
            }
            __hip_atomic_store(A.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch (stream order)
        }
    }
}

extern "C" int mi_xc_tail(mi_ctx *c, const double *d_w, const double *d_v0, const double *d_v1, const double *d_v2, int64_t ng,
                          double *d_tail, void *stream)
{
    if (!c || !d_w || !d_v0 || !d_tail || ng < 1) return fail("mi_xc_tail: bad argument");
    if (!c->d_xt_scratch) {
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(dev_malloc(&c->d_xt_scratch, sizeof(double) * (XT_MAXWG * 3 + 1)));
        HIPCHK(hipMemsetAsync(c->d_xt_scratch, 0, sizeof(double) * (XT_MAXWG * 3 + 1), (hipStream_t)stream));
    }
    XcTailArgs A{};
    A.w = d_w; A.v[0] = d_v0; A.v[1] = d_v1; A.v[2] = d_v2; A.nv = d_v2 ? 3 : (d_v1 ? 2 : 1); A.ng = ng; A.tail = d_tail;
    A.scratch = c->d_xt_scratch; A.ticket = reinterpret_cast<unsigned *>(c->d_xt_scratch + XT_MAXWG * 3);
    const int nwg = (int)std::max<int64_t>(1, std::min<int64_t>(XT_MAXWG, (ng + 2047) / 2048));
    hipLaunchKernelGGL(xc_tail_kernel, dim3(nwg), dim3(256), 0, (hipStream_t)stream, A);
    HIPCHK(hipGetLastError());
    return 0;
}

// Cholesky factor of M = G^T X G [nocc][nocc] (lower, row-major) and the triangular solve Zt = R^-1 W^T in ONE launch (replaces
// torch.linalg.cholesky_ex + solve_triangular: potf2, reset_info, iota, triu and trsm launches, 48 us per cycle at nocc = 21).
// W: [n][nocc] row-major; Zt: [nocc][n].  Every workgroup of 64 threads factors M itself in LDS (nocc <= 64: at most 90 k flops)
// and then solves for its 64 columns, row by row: z_i = (w_i - sum_{j<i} R_ij z_j) / R_ii with the earlier z_j kept in LDS.  info[0] = 0, or k + 1 for the first non-positive / non-finite pivot (LAPACK's convention);
// in that case Zt is filled with NaN so that the caller's electron count fails its check.
#define NYS_MAXOCC 64
__global__ __launch_bounds__(64) void nystrom_factor_kernel(const double *__restrict__ M, const double *__restrict__ W, int n, int nocc,
                                                            double *Zt, int *__restrict__ info)
{
    __shared__ double L[NYS_MAXOCC][NYS_MAXOCC + 1];
    __shared__ double zb[NYS_MAXOCC][64];
    __shared__ int fail_at;
    const int t = threadIdx.x;
    for (int idx = t; idx < nocc * nocc; idx += 64) { const int r = idx / nocc, c = idx - r * nocc; L[r][c] = M[idx]; }
    if (t == 0) fail_at = 0;
    __syncthreads();
    for (int k = 0; k < nocc; k++) {
        if (t == 0) {
            const double d = L[k][k];
            if (!(d > 0.0) || !isfinite(d)) { if (fail_at == 0) fail_at = k + 1; L[k][k] = 1.0; }
            else L[k][k] = sqrt(d);
        }
        __syncthreads();
        if (t > k && t < nocc) L[t][k] /= L[k][k];
        __syncthreads();
        const int m = nocc - k - 1;                       // trailing block (i, j), k < j <= i < nocc
        for (int idx = t; idx < m * m; idx += 64) {
            const int i = k + 1 + idx / m, j = k + 1 + idx % m;
            if (j <= i) L[i][j] = fma(-L[i][k], L[j][k], L[i][j]);
        }
        __syncthreads();
    }
    const bool failed = fail_at != 0;
    if (blockIdx.x == 0 && t == 0) info[0] = fail_at;
    const int c = blockIdx.x * 64 + t;
    if (c >= n) return;
    const double *w = W + (size_t)c * nocc;
    for (int i = 0; i < nocc; i++) {
        double z = w[i];
        for (int j = 0; j < i; j++) z = fma(-L[i][j], zb[j][t], z);    // this thread's earlier z_j: LDS column t, conflict-free
        z /= L[i][i];
        zb[i][t] = z;
        Zt[(size_t)i * n + c] = failed ? __builtin_nan("") : z;
    }
}

extern "C" int mi_nystrom_factor(mi_ctx *c, const double *d_M, const double *d_W, int n, int nocc, double *d_Zt, int *d_info, void *stream)
{
    if (!c || !d_M || !d_W || !d_Zt || !d_info || n < 1 || nocc < 1) return fail("mi_nystrom_factor: bad argument");
    if (nocc > NYS_MAXOCC) return fail("mi_nystrom_factor: at most %d columns", NYS_MAXOCC);
    hipLaunchKernelGGL(nystrom_factor_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, d_M, d_W, n, nocc, d_Zt, d_info);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int mi_nystrom_warm(mi_ctx *c, const double *d_Zt, const int *d_info, const double *d_G0, double *d_G, int nocc, int n,
                               void *stream)
{
    if (!c || !d_Zt || !d_info || !d_G0 || !d_G || nocc < 1 || n < 1) return fail("mi_nystrom_warm: bad argument");
    const int nb = (int)std::min<size_t>(64, ((size_t)nocc * n + 255) / 256);
    hipLaunchKernelGGL(nystrom_warm_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, d_Zt, d_info, d_G0, d_G, nocc, n);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int mi_xc_rho_mo(mi_ctx *c, const double *d_psi, int nocc, int64_t ng, int deriv, double *d_rho, double *d_tau, void *stream)
{
    if (!c) return fail("mi_xc_rho_mo: null context");
    if (ng < 0) return fail("mi_xc_rho_mo: negative number of grid points");
    if (nocc < 1 || (d_tau && !deriv)) return fail("mi_xc_rho_mo: bad argument");
    if (ng == 0) return 0;   // nothing to write (a zero-sized grid would be a launch error)
    if (!d_psi || !d_rho) return fail("mi_xc_rho_mo: null argument");
    hipLaunchKernelGGL(xc_rho_mo_kernel, dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_psi, nocc, ng, deriv, d_rho, d_tau);
    HIPCHK(hipGetLastError());
    return 0;
}

// The two steps above in ONE pass over the AO values, without psi ever leaving the registers: thread = grid point, the
// occupied orbitals in chunks of IC (4 IC accumulators: psi and its gradient), Z row by row through scalar loads
// (Zp[nao][ldz], orbital index fastest, zero-padded to a multiple of IC).  The AO values (the only large operand: 4 nao ng
// doubles) are streamed once per chunk, coalesced along the grid; rocBLAS needs 0.53 ms for the [21 x 264] x [264 x 123158]
// x 4 products alone (128-wide tiles on a 21-row output) where this kernel is bound by reading 1 GB of AO values.
template <int IC, bool DERIV>
__global__ __launch_bounds__(256) void xc_rho_lowrank_kernel(const double *__restrict__ ao, const double *__restrict__ Zp, int nao, int ldz,
                                                             int64_t ng, double *__restrict__ rho, double *__restrict__ tau)
{
    const int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t g = gi < ng ? gi : ng - 1;
    const size_t comp = (size_t)nao * ng;
    const MI_CONST_AS double *Zc = as_const(Zp);
    double r0 = 0, r1 = 0, r2 = 0, r3 = 0, tk = 0;
    for (int c0 = 0; c0 < ldz; c0 += IC) {
        double p0[IC], px[DERIV ? IC : 1], py[DERIV ? IC : 1], pz[DERIV ? IC : 1];
#pragma unroll
        for (int i = 0; i < IC; i++) { p0[i] = 0.0; if (DERIV) { px[i] = 0.0; py[i] = 0.0; pz[i] = 0.0; } }
#pragma unroll 2
        for (int m = 0; m < nao; m++) {
            const size_t o = (size_t)m * ng + g;
            const double a0 = ao[o];
            double ax = 0, ay = 0, az = 0;
            if (DERIV) { ax = ao[comp + o]; ay = ao[2 * comp + o]; az = ao[3 * comp + o]; }
            const MI_CONST_AS double *zr = Zc + (size_t)m * ldz + c0;
#pragma unroll
            for (int i = 0; i < IC; i++) {
                const double z = zr[i];
                p0[i] = fma(z, a0, p0[i]);
                if (DERIV) { px[i] = fma(z, ax, px[i]); py[i] = fma(z, ay, py[i]); pz[i] = fma(z, az, pz[i]); }
            }
        }
#pragma unroll
        for (int i = 0; i < IC; i++) {
            r0 = fma(p0[i], p0[i], r0);
            if (DERIV) {
                r1 = fma(px[i], p0[i], r1); r2 = fma(py[i], p0[i], r2); r3 = fma(pz[i], p0[i], r3);
                tk = fma(px[i], px[i], fma(py[i], py[i], fma(pz[i], pz[i], tk)));
            }
        }
    }
    if (gi >= ng) return;
    rho[g] = r0;
    if (DERIV) { rho[ng + g] = 2 * r1; rho[2 * ng + g] = 2 * r2; rho[3 * ng + g] = 2 * r3; if (tau) tau[g] = 0.5 * tk; }
}

// n_occ > 24 (ibuprofen: 56 -> three chunks) makes the kernel above walk the AO block once per chunk.  Tried and rejected (round 2,
// late): one wave per chunk over the same 64 grid points, partial densities added through LDS -- the AO block leaves HBM once, but
// the ibuprofen RKS cycle went from 27.3-29.5 to 32.9-34.0 ms (64-point workgroups, three waves contending for the same lines).
extern "C" int mi_xc_rho_lowrank(mi_ctx *c, const double *d_ao, const double *d_Zp, int ldz, int64_t ng, int deriv, double *d_rho,
                                 double *d_tau, void *stream)
{
    if (!c || !d_ao || !d_Zp || !d_rho || ldz < 1 || ng < 1 || (d_tau && !deriv)) return fail("mi_xc_rho_lowrank: bad argument");
    const dim3 g((unsigned)((ng + 255) / 256)), b(256);
    hipStream_t st = (hipStream_t)stream;
    if (deriv) {
        if (ldz % 24) return fail("mi_xc_rho_lowrank: ldz must be a multiple of 24 (GGA / meta-GGA chunk)");
        hipLaunchKernelGGL((xc_rho_lowrank_kernel<24, true>), g, b, 0, st, d_ao, d_Zp, c->nao, ldz, ng, d_rho, d_tau);
    } else {
        if (ldz % 32) return fail("mi_xc_rho_lowrank: ldz must be a multiple of 32 (LDA chunk)");
        hipLaunchKernelGGL((xc_rho_lowrank_kernel<32, false>), g, b, 0, st, d_ao, d_Zp, c->nao, ldz, ng, d_rho, d_tau);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- forward-mode dual numbers: value + N partial derivatives (N = 2: d/drho, d/dsigma of the closed-shell
// functionals; N = 5: d/d(rho_a, rho_b, sigma_aa, sigma_ab, sigma_bb) of the spin-polarised ones)
template <int N>
struct DN {
    double v, d[N];
    __device__ DN() {}
    __device__ DN(double a) : v(a) {
#pragma unroll
        for (int i = 0; i < N; i++) d[i] = 0.0;
    }
    __device__ static DN var(double a, int which) { DN x(a); x.d[which] = 1.0; return x; }
};
template <int N> __device__ inline DN<N> operator+(DN<N> a, DN<N> b) { DN<N> r; r.v = a.v + b.v;
#pragma unroll
    for (int i = 0; i < N; i++) r.d[i] = a.d[i] + b.d[i]; return r; }
template <int N> __device__ inline DN<N> operator-(DN<N> a, DN<N> b) { DN<N> r; r.v = a.v - b.v;
#pragma unroll
    for (int i = 0; i < N; i++) r.d[i] = a.d[i] - b.d[i]; return r; }
template <int N> __device__ inline DN<N> operator-(DN<N> a) { DN<N> r; r.v = -a.v;
#pragma unroll
    for (int i = 0; i < N; i++) r.d[i] = -a.d[i]; return r; }
template <int N> __device__ inline DN<N> operator*(DN<N> a, DN<N> b) { DN<N> r; r.v = a.v * b.v;
#pragma unroll
    for (int i = 0; i < N; i++) r.d[i] = a.d[i] * b.v + a.v * b.d[i]; return r; }
template <int N> __device__ inline DN<N> operator/(DN<N> a, DN<N> b) { DN<N> r; double iv = 1.0 / b.v, q = a.v * iv; r.v = q;
#pragma unroll
    for (int i = 0; i < N; i++) r.d[i] = (a.d[i] - q * b.d[i]) * iv; return r; }
template <int N> __device__ inline DN<N> chain(DN<N> a, double f, double df) { DN<N> r; r.v = f;
#pragma unroll
    for (int i = 0; i < N; i++) r.d[i] = df * a.d[i]; return r; }
template <int N> __device__ inline DN<N> dexp(DN<N> a) { double e = exp(a.v); return chain(a, e, e); }
template <int N> __device__ inline DN<N> dlog(DN<N> a) { return chain(a, log(a.v), 1.0 / a.v); }
template <int N> __device__ inline DN<N> dlog1p(DN<N> a) { return chain(a, log1p(a.v), 1.0 / (1.0 + a.v)); }
template <int N> __device__ inline DN<N> dsqrt(DN<N> a) { double s = sqrt(a.v); return chain(a, s, 0.5 / s); }
template <int N> __device__ inline DN<N> dpow(DN<N> a, double p) { double f = pow(a.v, p); return chain(a, f, p * f / a.v); }
template <int N> __device__ inline DN<N> datan(DN<N> a) { return chain(a, atan(a.v), 1.0 / (1.0 + a.v * a.v)); }
template <int N> __device__ inline DN<N> dasinh(DN<N> a) { return chain(a, asinh(a.v), rsqrt(1.0 + a.v * a.v)); }
template <int N> __device__ inline DN<N> derf(DN<N> a) { return chain(a, erf(a.v), 1.1283791670955126 * exp(-a.v * a.v)); } // 2/sqrt(pi) e^-x^2
typedef DN<2> D2;
typedef DN<5> D5;

// ---- second-order forward mode: value, gradient and Hessian (upper triangle packed row by row: (0,0), (0,1), .., (1,1), ..)
// in N variables, for the XC response kernels (mi_xc_fxc_prep).  The energy densities below instantiate with it unchanged.
template <int N>
struct HD {
    static constexpr int NH = N * (N + 1) / 2;
    double v, d[N], h[NH];
    __device__ HD() {}
    __device__ HD(double a) : v(a) {
#pragma unroll
        for (int i = 0; i < N; i++) d[i] = 0.0;
#pragma unroll
        for (int k = 0; k < NH; k++) h[k] = 0.0;
    }
    __device__ static HD var(double a, int which) { HD x(a); x.d[which] = 1.0; return x; }
    __device__ double hess(int i, int j) const { return h[i * N - i * (i - 1) / 2 + (j - i)]; }   // i <= j
};
template <int N> __device__ inline HD<N> operator+(HD<N> a, HD<N> b) { HD<N> r; r.v = a.v + b.v;
#pragma unroll
    for (int i = 0; i < N; i++) r.d[i] = a.d[i] + b.d[i];
#pragma unroll
    for (int k = 0; k < HD<N>::NH; k++) r.h[k] = a.h[k] + b.h[k]; return r; }
template <int N> __device__ inline HD<N> operator-(HD<N> a, HD<N> b) { HD<N> r; r.v = a.v - b.v;
#pragma unroll
    for (int i = 0; i < N; i++) r.d[i] = a.d[i] - b.d[i];
#pragma unroll
    for (int k = 0; k < HD<N>::NH; k++) r.h[k] = a.h[k] - b.h[k]; return r; }
template <int N> __device__ inline HD<N> operator-(HD<N> a) { HD<N> r; r.v = -a.v;
#pragma unroll
    for (int i = 0; i < N; i++) r.d[i] = -a.d[i];
#pragma unroll
    for (int k = 0; k < HD<N>::NH; k++) r.h[k] = -a.h[k]; return r; }
template <int N> __device__ inline HD<N> operator*(HD<N> a, HD<N> b) { HD<N> r; r.v = a.v * b.v;
#pragma unroll
    for (int i = 0; i < N; i++) r.d[i] = a.d[i] * b.v + a.v * b.d[i];
    int k = 0;
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = i; j < N; j++, k++) r.h[k] = a.h[k] * b.v + a.v * b.h[k] + a.d[i] * b.d[j] + a.d[j] * b.d[i];
    return r; }
// f(a) from f, f', f'' at a.v: d_i = f' a_i, h_ij = f' a_ij + f'' a_i a_j
template <int N> __device__ inline HD<N> chain2(HD<N> a, double f, double f1, double f2) { HD<N> r; r.v = f;
#pragma unroll
    for (int i = 0; i < N; i++) r.d[i] = f1 * a.d[i];
    int k = 0;
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = i; j < N; j++, k++) r.h[k] = f1 * a.h[k] + f2 * a.d[i] * a.d[j];
    return r; }
template <int N> __device__ inline HD<N> operator/(HD<N> a, HD<N> b) { double iv = 1.0 / b.v; return a * chain2(b, iv, -iv * iv, 2.0 * iv * iv * iv); }
template <int N> __device__ inline HD<N> dexp(HD<N> a) { double e = exp(a.v); return chain2(a, e, e, e); }
template <int N> __device__ inline HD<N> dlog(HD<N> a) { double iv = 1.0 / a.v; return chain2(a, log(a.v), iv, -iv * iv); }
template <int N> __device__ inline HD<N> dlog1p(HD<N> a) { double iv = 1.0 / (1.0 + a.v); return chain2(a, log1p(a.v), iv, -iv * iv); }
template <int N> __device__ inline HD<N> dsqrt(HD<N> a) { double s = sqrt(a.v); return chain2(a, s, 0.5 / s, -0.25 / (s * a.v)); }
template <int N> __device__ inline HD<N> dpow(HD<N> a, double p) { double f = pow(a.v, p), iv = 1.0 / a.v;
    return chain2(a, f, p * f * iv, p * (p - 1.0) * f * iv * iv); }
template <int N> __device__ inline HD<N> datan(HD<N> a) { double q = 1.0 / (1.0 + a.v * a.v); return chain2(a, atan(a.v), q, -2.0 * a.v * q * q); }
template <int N> __device__ inline HD<N> dasinh(HD<N> a) { double q = rsqrt(1.0 + a.v * a.v); return chain2(a, asinh(a.v), q, -a.v * q * q * q); }
template <int N> __device__ inline HD<N> derf(HD<N> a) { double g = 1.1283791670955126 * exp(-a.v * a.v); return chain2(a, erf(a.v), g, -2.0 * a.v * g); }

enum { XC_SLATER = 1, XC_B88 = 2, XC_VWN_RPA = 3, XC_VWN5 = 4, XC_LYP = 5, XC_PBE_X = 6, XC_PBE_C = 7,
       XC_TPSS_X = 8, XC_TPSS_C = 9, XC_M062X_X = 10, XC_M062X_C = 11,   // 8..11: meta-GGA (need tau)
       XC_B88_SR = 12 };   // short-range B88 (ITYH), GGA; needs its omega as the term's parameter
// functional ids a closed-shell or spin GGA evaluation accepts (mi_xc_eval*, mi_xc_eval_spin*)
__host__ inline bool xc_gga_kind(int k) { return (k >= XC_SLATER && k <= XC_PBE_C) || k == XC_B88_SR; }

// ---- closed-shell energy densities per volume e(rho, sigma); T is a dual-number type
template <class T> __device__ inline T f_slater(T rho) { return T(-0.7385587663820224) * dpow(rho, 4.0 / 3.0); } // -(3/4)(3/pi)^(1/3)

template <class T> __device__ inline T f_b88(T rho, T sig)
{
    const double beta = 0.0042;
    T rs = rho * T(0.5);                 // one spin channel
    T r43 = dpow(rs, 4.0 / 3.0);
    T x = dsqrt(sig * T(0.25) + T(1e-300)) / r43;
    T corr = T(-beta) * r43 * x * x / (T(1.0) + T(6.0 * beta) * x * dasinh(x));
    return f_slater(rho) + T(2.0) * corr;
}

// ITYH attenuation (Iikura, Tsuneda, Yanai, Hirao, JCP 115, 3540 (2001)) of one spin channel's exchange by erfc(omega r12):
//   F(a) = 1 - 8/3 a [sqrt(pi) erf(1/(2a)) + (2a - 4a^3) exp(-1/(4a^2)) - 3a + 4a^3],  a = omega / (2 k_sigma).
// The bracket cancels in FP64 as a grows (relative error of F ~1e-11 at a = 2..4, 4e-10 at 5, 3 % at 100; low-density grid
// points reach a ~ 100 and beyond), so from a = 1 on the series in 1/a^2 is used.  It converges for every a (F is entire in
// 1/a); twelve terms truncate below 1e-16 of F + a F'/2 at a = 1.  The energy density needs K F(a) with a^2 proportional to K,
// and de/dsigma = K' (F + a F'/2), in which the leading 1/(36a^2) terms cancel and leave 1e-2 (a = 1) .. 1e-7 (a ~ 1000) of
// F.  The series branch therefore returns P(u) = F(a)/u, u = 1/a^2, and the caller multiplies by K u = K/a^2, which it forms
// without K: the leading term then has a derivative in sigma of exactly zero and nothing cancels.  Below the switch the
// closed form keeps F + a F'/2 to ~1e-12 relative (bracket terms <= 4 against a result of 0.36 at a = 1).
#define ITYH_SERIES_A 1.0
template <class T> __device__ inline T ityh_closed(T a)
{
    const T a2 = a * a, a3 = a2 * a;
    return T(1.0) - T(8.0 / 3.0) * a * (T(1.7724538509055159) * derf(T(0.5) / a) + (T(2.0) * a - T(4.0) * a3) * dexp(T(-0.25) / a2)
                                        - T(3.0) * a + T(4.0) * a3);
}
// P(u) = F(a) a^2 at u = 1/a^2: 1/36 - u/960 + u^2/26880 - ...
template <class T> __device__ inline T ityh_series_over_u(T u)
{
    const double c[12] = {1.0 / 36.0, 1.0 / 960.0, 1.0 / 26880.0, 1.0 / 829440.0, 1.0 / 28385280.0, 1.0 / 1073479680.0,
                          1.0 / 44590694400.0, 1.0 / 2021444812800.0, 1.0 / 99407521382400.0, 1.0 / 5273830608076800.0,
                          1.0 / 300357209869516800.0, 1.0 / 18282612774666240000.0};
    T p(c[11]);
#pragma unroll
    for (int k = 10; k >= 0; k--) p = T(c[k]) - u * p;
    return p;
}

// Short-range B88 of CAM-B3LYP, closed shell: per spin channel e_s^SR = e_s^B88 F(a_s) with e_s^B88 = -1/2 rho_s^(4/3) K_s (Slater
// included, as f_b88), k_s = sqrt(9 pi / K_s) rho_s^(1/3), a_s = omega / (2 k_s), i.e. a_s^2 = q K_s with q = omega^2 /
// (36 pi rho_s^(2/3)).  omega > 0 (checked by the entry points).
template <class T> __device__ inline T f_b88_sr(T rho, T sig, double omega)
{
    const double beta = 0.0042;
    T rs = rho * T(0.5);                 // one spin channel
    T r13 = dpow(rs, 1.0 / 3.0), r43 = rs * r13;
    T x = dsqrt(sig * T(0.25) + T(1e-300)) / r43;
    T K = T(1.8610514726982001) /* 3/2 (6/pi)^(1/3) */ + T(2.0 * beta) * x * x / (T(1.0) + T(6.0 * beta) * x * dasinh(x));
    T q = T(omega * omega / (36.0 * M_PI)) / (r13 * r13);
    T a2 = q * K;
    if (a2.v >= ITYH_SERIES_A * ITYH_SERIES_A) return -(r43 / q * ityh_series_over_u(T(1.0) / a2));  // K F = (K u) P(u), K u = 1/q
    return -(r43 * K * ityh_closed(dsqrt(a2)));  // 2 e_s^SR
}

// VWN fit: correlation energy per electron as a function of x = sqrt(rs)
template <class T> __device__ inline T vwn_eps(T x, double A, double x0, double b, double c)
{
    T X = x * x + T(b) * x + T(c);
    double X0 = x0 * x0 + b * x0 + c, Q = sqrt(4 * c - b * b);
    T at = datan(T(Q) / (T(2.0) * x + T(b)));
    T xm = x - T(x0);
    return T(A) * (dlog(x * x / X) + T(2 * b / Q) * at - T(b * x0 / X0) * (dlog(xm * xm / X) + T(2 * (b + 2 * x0) / Q) * at));
}

template <class T> __device__ inline T f_vwn(T rho, double A, double x0, double b, double c)
{
    T rs = dpow(T(0.75 / M_PI) / rho, 1.0 / 3.0);
    return rho * vwn_eps(dsqrt(rs), A, x0, b, c);
}

template <class T> __device__ inline T f_lyp(T rho, T sig)
{
    const double a = 0.04918, b = 0.132, c = 0.2533, d = 0.349;
    const double CF = 2.871234000188191; // (3/10)(3 pi^2)^(2/3)
    T t = dpow(rho, -1.0 / 3.0);
    T Dn = T(1.0) + T(d) * t;
    T om = dexp(T(-c) * t) / Dn * dpow(rho, -11.0 / 3.0);
    T dl = T(c) * t + T(d) * t / Dn;
    T br = T(CF) * dpow(rho, 14.0 / 3.0) - rho * rho * sig * (T(1.0 / 24.0) + T(7.0 / 72.0) * dl);
    return T(-a) * rho / Dn - T(a * b) * om * br;
}

template <class T> __device__ inline T f_pbe_x(T rho, T sig)
{
    const double kappa = 0.804, mu = 0.06672455060314922 * M_PI * M_PI / 3.0;
    T kf = dpow(T(3.0 * M_PI * M_PI) * rho, 1.0 / 3.0);
    T s2 = sig / (T(4.0) * kf * kf * rho * rho);
    T F = T(1.0 + kappa) - T(kappa) / (T(1.0) + T(mu / kappa) * s2);
    return f_slater(rho) * F;
}

// PW92 form G(rs; A, a1, b1..b4) = -2A(1 + a1 rs) ln(1 + 1/(2A(b1 x + b2 x^2 + b3 x^3 + b4 x^4))), x = sqrt(rs)
template <class T> __device__ inline T pw92_g(T rs, double A, double a1, double b1, double b2, double b3, double b4)
{
    T x = dsqrt(rs);
    // log1p: the argument is 1e-5 in the density tail (rs ~ 1e3), where log(1 + .) keeps 11 digits only
    return T(-2 * A) * (T(1.0) + T(a1) * rs) * dlog1p(T(1.0) / (T(2 * A) * (T(b1) * x + T(b2) * rs + T(b3) * rs * x + T(b4) * rs * rs)));
}

// eps_c + H of PBE correlation, H = g log(1 + (beta/gamma) t^2 (1 + y) / (1 + y + y^2)), g = gamma phi^3, y = A t^2,
// A = (beta/gamma) / E1, E1 = exp(-eps_c / g) - 1.  At large reduced gradients y(1 + y)/(1 + y + y^2) -> 1 and H -> -eps_c:
// the quotient rule then forms the derivative (1 + 2y)/(1 + y + y^2)^2 as a difference of two numbers y^2 times larger, and
// eps_c + H cancels (y reaches 1e10 in density tails; de/dsigma and the second derivatives lost every digit there).  With
// -eps_c = g log(1 + E1) the sum is g log(1 - E1/(1 + E1) / (1 + y + y^2)) exactly, in which nothing cancels; it is used
// from y = 1 on, where the plain form is still well conditioned.
template <class T> __device__ inline T pbe_c_eps_plus_h(T ec, T g, T t2)
{
    const double bg = 0.06672455060314922 / 0.031090690869654895;
    T E1 = dexp(-ec / g) - T(1.0);
    T y = T(bg) / E1 * t2;
    T D = T(1.0) + y + y * y;
    if (y.v > 1.0) return g * dlog1p(-(E1 / (T(1.0) + E1)) / D);
    return ec + g * dlog(T(1.0) + T(bg) * t2 * (T(1.0) + y) / D);
}

template <class T> __device__ inline T f_pbe_c(T rho, T sig)
{
    const double gamma = 0.031090690869654895;
    T rs = dpow(T(0.75 / M_PI) / rho, 1.0 / 3.0);
    T ec = pw92_g(rs, 0.031090690869654895, 0.21370, 7.5957, 3.5876, 1.6382, 0.49294);
    T kf = dpow(T(3.0 * M_PI * M_PI) * rho, 1.0 / 3.0);
    T ks2 = T(4.0 / M_PI) * kf;
    T t2 = sig / (T(4.0) * ks2 * rho * rho);
    return rho * pbe_c_eps_plus_h(ec, T(gamma), t2);
}

// ---- spin-polarised forms e(rho_a, rho_b, sigma_aa, sigma_ab, sigma_bb)
// A spin channel is evaluated from XC_CHANNEL_FLOOR up.  The floor only keeps rho_s^(4/3) and the reduced gradient away from
// underflow and 0/0.  What it drops is largest in M06-2X's opposite-spin correlation, which is linear in the minority density:
// ~5 rho_s |eps_c| with eps_c ~ 1e-4 at rho = 1e-10, against 1e-11 of the LDA exchange 0.74 rho^(4/3) = 3e-14 of a point that
// just passes the density cut-off of the kernels (rho_a + rho_b > 1e-10): rho_s < 6e-22.  Exchange drops (rho_s / rho)^(4/3).
// (A floor of 1e-12 dropped 1e-4 of the LDA exchange at rho_a = 1e-9.)
#define XC_CHANNEL_FLOOR 1e-24
// exchange: spin scaling  E_x[ra, rb] = (E_x[2 ra] + E_x[2 rb]) / 2  with sigma -> 4 sigma_ss
template <class T, class F> __device__ inline T spin_scaled_exchange(T ra, T rb, T saa, T sbb, F fx)
{
    T e(0.0);
    if (ra.v > XC_CHANNEL_FLOOR) e = e + T(0.5) * fx(T(2.0) * ra, T(4.0) * saa);
    if (rb.v > XC_CHANNEL_FLOOR) e = e + T(0.5) * fx(T(2.0) * rb, T(4.0) * sbb);
    return e;
}
// zeta = (ra - rb)/rho clipped away from +-1, for TPSS correlation's C(zeta, xi) alone: its (1 +- zeta)^(-4/3) stays finite
// (1e20 at the clip) and multiplies xi^2, which vanishes with the minority gradient.  A clip at 1 - 1e-10 moved C(zeta, 0) of
// every fully polarised point by 1e-9; the spin interpolations f(zeta) and phi(zeta) do not go through here (spin_pow_sum).
template <class T> __device__ inline T spin_zeta(T ra, T rb)
{
    T z = (ra - rb) / (ra + rb);
    const double lim = 1.0 - 1e-15;
    if (z.v > lim) z = T(lim);
    if (z.v < -lim) z = T(-lim);
    return z;
}
// (1 + zeta)^p + (1 - zeta)^p, p > 0, from 1 +- zeta = 2 rho_s / rho: the spin interpolations keep the digits of a nearly
// empty channel, which zeta = (ra - rb)/rho rounds away and its clip replaces (phi of PBE correlation holds (1 - zeta)^(2/3):
// a clip at 1 - d moves it by d^(2/3), 1e-10 even for d = 1e-15).  An empty channel contributes its limit, 0.
template <class T> __device__ inline T spin_pow_sum(T ra, T rb, double p)
{
    T rho = ra + rb, s(0.0);
    if (ra.v > 0.0) s = s + dpow(T(2.0) * ra / rho, p);
    if (rb.v > 0.0) s = s + dpow(T(2.0) * rb / rho, p);
    return s;
}
template <class T> __device__ inline T spin_fzeta(T ra, T rb) // ((1+z)^(4/3) + (1-z)^(4/3) - 2) / (2^(4/3) - 2)
{
    return (spin_pow_sum(ra, rb, 4.0 / 3.0) - T(2.0)) * T(1.0 / (2.5198420997897464 - 2.0));
}
template <class T> __device__ inline T spin_zeta4(T ra, T rb) { T z = (ra - rb) / (ra + rb), z2 = z * z; return z2 * z2; }
// VWN-RPA (libxc LDA_C_VWN_RPA, the correlation of B3LYP): eps = eps_P + (eps_F - eps_P) f(zeta), RPA fits
template <class T> __device__ inline T f_vwn_rpa_spin(T ra, T rb)
{
    T rho = ra + rb;
    T x = dsqrt(dpow(T(0.75 / M_PI) / rho, 1.0 / 3.0));
    T eP = vwn_eps(x, 0.0310907, -0.409286, 13.0720, 42.7198);
    T eF = vwn_eps(x, 0.01554535, -0.743294, 20.1231, 101.578);
    return rho * (eP + (eF - eP) * spin_fzeta(ra, rb));
}
// VWN5: eps = eps_P + alpha_c f(z)/f''(0) (1 - z^4) + (eps_F - eps_P) f(z) z^4
template <class T> __device__ inline T f_vwn5_spin(T ra, T rb)
{
    T rho = ra + rb;
    T x = dsqrt(dpow(T(0.75 / M_PI) / rho, 1.0 / 3.0));
    T eP = vwn_eps(x, 0.0310907, -0.10498, 3.72744, 12.9352);
    T eF = vwn_eps(x, 0.01554535, -0.32500, 7.06042, 18.0578);
    T ac = vwn_eps(x, -1.0 / (6.0 * M_PI * M_PI), -0.0047584, 1.13107, 13.0045);
    T fz = spin_fzeta(ra, rb), z4 = spin_zeta4(ra, rb);
    return rho * (eP + ac * fz * T(1.0 / 1.7099209341613657) * (T(1.0) - z4) + (eF - eP) * fz * z4);
}
// LYP, open-shell form of Miehlich, Savin, Stoll, Preuss, CPL 157, 200 (1989)
template <class T> __device__ inline T f_lyp_spin(T ra, T rb, T saa, T sab, T sbb)
{
    const double a = 0.04918, b = 0.132, c = 0.2533, d = 0.349;
    const double CF = 2.871234000188191;
    T rho = ra + rb;
    T sig = saa + T(2.0) * sab + sbb;
    T t = dpow(rho, -1.0 / 3.0);
    T Dn = T(1.0) + T(d) * t;
    T om = dexp(T(-c) * t) / Dn * dpow(rho, -11.0 / 3.0);
    T dl = T(c) * t + T(d) * t / Dn;
    T rab = ra * rb;
    T pa(0.0), pb(0.0);
    if (ra.v > 1e-14) pa = dpow(ra, 8.0 / 3.0);
    if (rb.v > 1e-14) pb = dpow(rb, 8.0 / 3.0);
    T t1 = T(12.699208415745595 * CF) * (pa + pb) /* 2^(11/3) C_F */ + (T(47.0 / 18.0) - T(7.0 / 18.0) * dl) * sig -
           (T(2.5) - dl * T(1.0 / 18.0)) * (saa + sbb) - (dl - T(11.0)) * T(1.0 / 9.0) * (ra / rho * saa + rb / rho * sbb);
    T br = rab * t1 - T(2.0 / 3.0) * rho * rho * sig + (T(2.0 / 3.0) * rho * rho - ra * ra) * sbb + (T(2.0 / 3.0) * rho * rho - rb * rb) * saa;
    return T(-4.0 * a) * rab / (Dn * rho) - T(a * b) * om * br;
}
// PBE correlation with the PW92 spin interpolation and phi(zeta)
template <class T> __device__ inline T f_pbe_c_spin(T ra, T rb, T saa, T sab, T sbb)
{
    const double gamma = 0.031090690869654895;
    T rho = ra + rb;
    T sig = saa + T(2.0) * sab + sbb;
    T rs = dpow(T(0.75 / M_PI) / rho, 1.0 / 3.0);
    T e0 = pw92_g(rs, 0.031090690869654895, 0.21370, 7.5957, 3.5876, 1.6382, 0.49294);
    T e1 = pw92_g(rs, 0.015545345434827448, 0.20548, 14.1189, 6.1977, 3.3662, 0.62517);
    T mac = pw92_g(rs, 0.016886863940389627, 0.11125, 10.357, 3.6231, 0.88026, 0.49671); // = -alpha_c
    T fz = spin_fzeta(ra, rb), z4 = spin_zeta4(ra, rb);
    T ec = e0 - mac * fz * T(1.0 / 1.7099209341613657) * (T(1.0) - z4) + (e1 - e0) * fz * z4;
    T phi = T(0.5) * spin_pow_sum(ra, rb, 2.0 / 3.0);
    T phi3 = phi * phi * phi;
    T kf = dpow(T(3.0 * M_PI * M_PI) * rho, 1.0 / 3.0);
    T ks2 = T(4.0 / M_PI) * kf;
    T t2 = sig / (T(4.0) * phi * phi * ks2 * rho * rho);
    return rho * pbe_c_eps_plus_h(ec, T(gamma) * phi3, t2);
}

// =================================================================================================
// meta-GGA functionals (`--method M06-2X` at templates/calculate_energy.py:263, the default of
// templates/calculate_bde.py:105,502).  Spin-resolved energy densities per volume e(rho_a, rho_b, sigma_aa, sigma_ab,
// sigma_bb, tau_a, tau_b), tau_s = 1/2 sum_i |grad phi_i,s|^2, coded once on the dual-number type; the closed-shell kernel
// calls them with rho_s = rho/2, sigma_ss' = sigma/4, tau_s = tau/2.
//   TPSS      Tao, Perdew, Staroverov, Scuseria, PRL 91, 146401 (2003): exchange eq. 10, correlation = revPKZB (eqs. 11-14)
//   M06-2X    Zhao, Truhlar, Theor. Chem. Acc. 120, 215 (2008): PBE-exchange x kinetic-energy-density series (the VS98-type
//             exchange term is zero for M06-2X), M05-type + VS98-type correlation; 54 % exact exchange.
// PARAMETER TABLES ENTERED FROM MEMORY (no libxc here): "unverified-memory".  What IS checked (tests): the uniform-gas limit
// (a_0 + X = 1, c_0 + d_0 = 1 for both correlation channels), vanishing correlation and the exact TPSS exchange energy for
// one-electron densities, derivatives against the complex-step oracle.
// =================================================================================================
template <class T> __device__ inline T dmaxv(T a, T b) { return a.v >= b.v ? a : b; }

// PW92 correlation energy per particle of the spin-polarised uniform gas
template <class T> __device__ inline T pw92_eps_spin(T ra, T rb)
{
    T rho = ra + rb;
    T rs = dpow(T(0.75 / M_PI) / rho, 1.0 / 3.0);
    T e0 = pw92_g(rs, 0.031090690869654895, 0.21370, 7.5957, 3.5876, 1.6382, 0.49294);
    T e1 = pw92_g(rs, 0.015545345434827448, 0.20548, 14.1189, 6.1977, 3.3662, 0.62517);
    T mac = pw92_g(rs, 0.016886863940389627, 0.11125, 10.357, 3.6231, 0.88026, 0.49671);
    T fz = spin_fzeta(ra, rb), z4 = spin_zeta4(ra, rb);
    return e0 - mac * fz * T(1.0 / 1.7099209341613657) * (T(1.0) - z4) + (e1 - e0) * fz * z4;
}

// ---- TPSS exchange of a spin-UNpolarised density (rho, sigma = |grad rho|^2, tau); spin scaling handles the rest
template <class T> __device__ inline T f_tpss_x_unpol(T rho, T sig, T tau)
{
    const double kappa = 0.804, bb = 0.40, cc = 1.59096, ee = 1.537, mu = 0.21951, se = 1.2397580409105368 /* sqrt(e) */;
    T p = sig / (T(4.0 * 9.570780000627305 /* (3 pi^2)^(2/3) */) * dpow(rho, 8.0 / 3.0));
    T tw = sig / (T(8.0) * rho);
    T z = tw / tau;
    if (z.v > 1.0) z = T(1.0);                                   // tau_W <= tau for N-representable input
    T tunif = T(0.3 * 9.570780000627305) * dpow(rho, 5.0 / 3.0);
    T alpha = (tau - tw) / tunif;
    if (alpha.v < 0.0) alpha = T(0.0);
    T qb = T(0.45) * (alpha - T(1.0)) / dsqrt(T(1.0) + T(bb) * alpha * (alpha - T(1.0))) + T(2.0 / 3.0) * p;
    T z2 = z * z;
    T t1 = (T(10.0 / 81.0) + T(cc) * z2 / ((T(1.0) + z2) * (T(1.0) + z2))) * p;
    T t2 = T(146.0 / 2025.0) * qb * qb;
    T t3 = T(-73.0 / 405.0) * qb * dsqrt(T(0.5) * (T(0.6) * z) * (T(0.6) * z) + T(0.5) * p * p + T(1e-300));
    T t4 = T((10.0 / 81.0) * (10.0 / 81.0) / kappa) * p * p;
    T t5 = T(2.0 * se * (10.0 / 81.0)) * (T(0.6) * z) * (T(0.6) * z);
    T t6 = T(ee * mu) * p * p * p;
    T den = T(1.0) + T(se) * p;
    T x = (t1 + t2 + t3 + t4 + t5 + t6) / (den * den);
    T Fx = T(1.0 + kappa) - T(kappa) / (T(1.0) + x / T(kappa));
    return f_slater(rho) * Fx;
}
template <class T> __device__ inline T f_tpss_x_spin(T ra, T rb, T saa, T sbb, T ta, T tb)
{
    T e(0.0);
    // tau_s > 0 is all the formula needs (z = tau_W / tau may overflow to inf, which the clip z <= 1 takes); the uniform-gas
    // tau of a tail point is far below any fixed threshold (2.9 rho^(5/3) = 3e-15 at rho = 1e-9)
    if (ra.v > XC_CHANNEL_FLOOR && ta.v > 0.0) e = e + T(0.5) * f_tpss_x_unpol(T(2.0) * ra, T(4.0) * saa, T(2.0) * ta);
    if (rb.v > XC_CHANNEL_FLOOR && tb.v > 0.0) e = e + T(0.5) * f_tpss_x_unpol(T(2.0) * rb, T(4.0) * sbb, T(2.0) * tb);
    return e;
}
// ---- TPSS correlation (revPKZB)
template <class T> __device__ inline T f_tpss_c_spin(T ra, T rb, T saa, T sab, T sbb, T ta, T tb)
{
    const double d = 2.8;
    T rho = ra + rb, sig = saa + T(2.0) * sab + sbb, tau = ta + tb;
    if (!(tau.v > 0.0)) return T(0.0);
    T tw = sig / (T(8.0) * rho);
    T z = tw / tau;
    if (z.v > 1.0) z = T(1.0);
    T zeta = spin_zeta(ra, rb);
    // xi = |grad zeta| / (2 (3 pi^2 rho)^(1/3)),  |grad zeta|^2 = 4 (rb^2 saa - 2 ra rb sab + ra^2 sbb) / rho^4
    T gz2 = T(4.0) * (rb * rb * saa - T(2.0) * ra * rb * sab + ra * ra * sbb) / (rho * rho * rho * rho);
    if (gz2.v < 0.0) gz2 = T(0.0);
    T xi2 = gz2 / (T(4.0) * dpow(T(3.0 * M_PI * M_PI) * rho, 2.0 / 3.0));
    T z2_ = zeta * zeta;
    T C0 = T(0.53) + T(0.87) * z2_ + T(0.50) * z2_ * z2_ + T(2.26) * z2_ * z2_ * z2_;
    T den = T(1.0) + xi2 * T(0.5) * (dpow(T(1.0) + zeta, -4.0 / 3.0) + dpow(T(1.0) - zeta, -4.0 / 3.0));
    T den2 = den * den;
    T C = C0 / (den2 * den2);
    T epbe = f_pbe_c_spin(ra, rb, saa, sab, sbb) / rho;
    T ea = epbe, eb = epbe;
    if (ra.v > XC_CHANNEL_FLOOR) ea = dmaxv(f_pbe_c_spin(ra, T(0.0), saa, T(0.0), T(0.0)) / ra, epbe);
    if (rb.v > XC_CHANNEL_FLOOR) eb = dmaxv(f_pbe_c_spin(rb, T(0.0), sbb, T(0.0), T(0.0)) / rb, epbe);
    T zz = z * z;
    T erev = epbe * (T(1.0) + C * zz) - (T(1.0) + C) * zz * (ra / rho * ea + rb / rho * eb);
    return rho * erev * (T(1.0) + T(d) * erev * zz * z);
}

// ---- M06-2X.  Parameter tables: unverified-memory (see the header of this block).
__device__ __constant__ double M062X_A[12] = {4.600000e-01, -2.206052e-01, -9.431788e-02, 2.164494e+00, -2.556466e+00, -1.422133e+01,
                                              1.555044e+01, 3.598078e+01, -2.722754e+01, -3.924093e+01, 1.522808e+01, 1.522227e+01};
__device__ __constant__ double M062X_CSS[5] = {3.097855e-01, -5.528642e+00, 1.347420e+01, -3.213623e+01, 2.846742e+01};
__device__ __constant__ double M062X_CAB[5] = {8.833596e-01, 3.357972e+01, -7.043548e+01, 4.978271e+01, -1.852891e+01};
__device__ __constant__ double M062X_DSS[6] = {6.902145e-01, 9.847204e-02, 2.214797e-01, -1.968264e-03, -6.775479e-03, 0.0};
__device__ __constant__ double M062X_DAB[6] = {1.166404e-01, -9.120847e-02, -6.726189e-02, 6.720580e-05, 8.448011e-04, 0.0};
#define M06_CF 9.115599744691194 /* (3/5)(6 pi^2)^(2/3) */

template <class T> __device__ inline T f_m06_x_channel(T r, T s, T tau, const double *a) // one spin channel: r = rho_s
{
    T tl = T(0.3 * 15.192666241151989 /* (6 pi^2)^(2/3) */) * dpow(r, 5.0 / 3.0);
    T w = (tl - tau) / (tl + tau);          // (t - 1)/(t + 1) with t = tau_LDA / tau, without the quotient that overflows
    T fw(a[11]);
#pragma unroll
    for (int i = 10; i >= 0; i--) fw = fw * w + T(a[i]);
    return T(0.5) * f_pbe_x(T(2.0) * r, T(4.0) * s) * fw;
}
template <class T> __device__ inline T f_m062x_x_spin(T ra, T rb, T saa, T sbb, T ta, T tb)
{
    T e(0.0);
    if (ra.v > XC_CHANNEL_FLOOR && ta.v > 0.0) e = e + f_m06_x_channel(ra, saa, ta, M062X_A);
    if (rb.v > XC_CHANNEL_FLOOR && tb.v > 0.0) e = e + f_m06_x_channel(rb, sbb, tb, M062X_A);
    return e;
}
template <class T> __device__ inline T m06_h(T x2, T z, const double *dc, double alpha)
{
    T g = T(1.0) + T(alpha) * (x2 + z);
    return T(dc[0]) / g + (T(dc[1]) * x2 + T(dc[2]) * z) / (g * g) + (T(dc[3]) * x2 * x2 + T(dc[4]) * x2 * z + T(dc[5]) * z * z) / (g * g * g);
}
template <class T> __device__ inline T m06_g(T x2, const double *cc, double gamma)
{
    T u = T(gamma) * x2 / (T(1.0) + T(gamma) * x2);
    T g(cc[4]);
#pragma unroll
    for (int i = 3; i >= 0; i--) g = g * u + T(cc[i]);
    return g;
}
template <class T> __device__ inline T f_m062x_c_spin(T ra, T rb, T saa, T sbb, T ta, T tb)
{
    const bool ha = ra.v > XC_CHANNEL_FLOOR && ta.v > 0.0, hb = rb.v > XC_CHANNEL_FLOOR && tb.v > 0.0;
    T e(0.0), ess_a(0.0), ess_b(0.0), x2a(0.0), x2b(0.0), za(0.0), zb(0.0);
    if (ha) {
        x2a = saa / dpow(ra, 8.0 / 3.0);
        za = T(2.0) * ta / dpow(ra, 5.0 / 3.0) - T(M06_CF);
        ess_a = ra * pw92_eps_spin(ra, T(0.0));
        T Dsic = T(1.0) - saa / (T(8.0) * ra * ta);   // 1 - x^2 / (4 (z + C_F)) = 1 - tau_W / tau, without the detour (z - C_F) + C_F
        if (Dsic.v < 0.0) Dsic = T(0.0);
        e = e + ess_a * (m06_g(x2a, M062X_CSS, 0.06) + m06_h(x2a, za, M062X_DSS, 0.00515088)) * Dsic;
    }
    if (hb) {
        x2b = sbb / dpow(rb, 8.0 / 3.0);
        zb = T(2.0) * tb / dpow(rb, 5.0 / 3.0) - T(M06_CF);
        ess_b = rb * pw92_eps_spin(rb, T(0.0));
        T Dsic = T(1.0) - sbb / (T(8.0) * rb * tb);
        if (Dsic.v < 0.0) Dsic = T(0.0);
        e = e + ess_b * (m06_g(x2b, M062X_CSS, 0.06) + m06_h(x2b, zb, M062X_DSS, 0.00515088)) * Dsic;
    }
    if (ha && hb) {
        T eab = (ra + rb) * pw92_eps_spin(ra, rb) - ess_a - ess_b;
        e = e + eab * (m06_g(x2a + x2b, M062X_CAB, 0.0031) + m06_h(x2a + x2b, za + zb, M062X_DAB, 0.00304966));
    }
    return e;
}

struct XcSpec { int n; int kind[8]; double coef[8]; double param[8]; };   // param: omega of an XC_B88_SR term

// sum_t coef_t e_t of the GGA terms of X: closed shell over (rho, sigma), spin-polarised over (rho_a, rho_b, sigma_aa, sigma_ab,
// sigma_bb).  T is a first-order (DN) or second-order (HD) dual-number type.
template <class T> __device__ inline T xc_closed_sum(const XcSpec &X, T R, T S)
{
    T acc(0.0);
    for (int t = 0; t < X.n; t++) {
        T f;
        switch (X.kind[t]) {
        case XC_SLATER: f = f_slater(R); break;
        case XC_B88: f = f_b88(R, S); break;
        case XC_VWN_RPA: f = f_vwn(R, 0.0310907, -0.409286, 13.0720, 42.7198); break;
        case XC_VWN5: f = f_vwn(R, 0.0310907, -0.10498, 3.72744, 12.9352); break;
        case XC_LYP: f = f_lyp(R, S); break;
        case XC_PBE_X: f = f_pbe_x(R, S); break;
        case XC_PBE_C: f = f_pbe_c(R, S); break;
        case XC_B88_SR: f = f_b88_sr(R, S, X.param[t]); break;
        default: f = T(0.0);
        }
        acc = acc + T(X.coef[t]) * f;
    }
    return acc;
}

// One spin-polarised term e_t(rho_a, rho_b, sigma_aa, sigma_ab, sigma_bb, tau_a, tau_b): the only spin dispatch, behind every
// kernel that evaluates the spin forms.  MGGA compiles the meta-GGA terms in; without it they are not instantiated (the GGA
// kernels and the second-order duals of xc_fxc_prep_kernel keep their registers) and the taus are dead.
template <bool MGGA, class T>
__device__ inline T xc_term_spin(int kind, double prm, T Ra, T Rb, T Saa, T Sab, T Sbb, T Ta, T Tb)
{
    switch (kind) {
    case XC_SLATER: return spin_scaled_exchange(Ra, Rb, Saa, Sbb, [](T r, T) { return f_slater(r); });
    case XC_B88: return spin_scaled_exchange(Ra, Rb, Saa, Sbb, [](T r, T s_) { return f_b88(r, s_); });
    case XC_PBE_X: return spin_scaled_exchange(Ra, Rb, Saa, Sbb, [](T r, T s_) { return f_pbe_x(r, s_); });
    case XC_B88_SR: return spin_scaled_exchange(Ra, Rb, Saa, Sbb, [prm](T r, T s_) { return f_b88_sr(r, s_, prm); });
    case XC_VWN_RPA: return f_vwn_rpa_spin(Ra, Rb);
    case XC_VWN5: return f_vwn5_spin(Ra, Rb);
    case XC_LYP: return f_lyp_spin(Ra, Rb, Saa, Sab, Sbb);
    case XC_PBE_C: return f_pbe_c_spin(Ra, Rb, Saa, Sab, Sbb);
    default: break;
    }
    if constexpr (MGGA) {
        switch (kind) {
        case XC_TPSS_X: return f_tpss_x_spin(Ra, Rb, Saa, Sbb, Ta, Tb);
        case XC_TPSS_C: return f_tpss_c_spin(Ra, Rb, Saa, Sab, Sbb, Ta, Tb);
        case XC_M062X_X: return f_m062x_x_spin(Ra, Rb, Saa, Sbb, Ta, Tb);
        case XC_M062X_C: return f_m062x_c_spin(Ra, Rb, Saa, Sbb, Ta, Tb);
        default: break;
        }
    }
    return T(0.0);
}

template <bool MGGA = false, class T>
__device__ inline T xc_spin_sum(const XcSpec &X, T Ra, T Rb, T Saa, T Sab, T Sbb, T Ta = T(0.0), T Tb = T(0.0))
{
    T acc(0.0);
    for (int t = 0; t < X.n; t++) acc = acc + T(X.coef[t]) * xc_term_spin<MGGA>(X.kind[t], X.param[t], Ra, Rb, Saa, Sab, Sbb, Ta, Tb);
    return acc;
}

// exc[g] = e(rho,sigma) per volume; wv[0] = 0.5 w de/drho ; wv[1..3] = 2 w de/dsigma * grad rho
__global__ __launch_bounds__(256) void xc_eval_kernel(XcSpec X, const double *rho, const double *w, int64_t ng, int gga,
                                                      double *exc, double *wv, double *vrho_out, double *vsig_out)
{
    int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ng) return;
    double r = rho[g];
    double gx = gga ? rho[ng + g] : 0.0, gy = gga ? rho[2 * ng + g] : 0.0, gz = gga ? rho[3 * ng + g] : 0.0;
    double e = 0.0, vr = 0.0, vs = 0.0;
    if (r > 1e-10) {
        D2 acc = xc_closed_sum(X, D2::var(r, 0), D2::var(gx * gx + gy * gy + gz * gz, 1));
        e = acc.v; vr = acc.d[0]; vs = acc.d[1];
    }
    if (exc) exc[g] = e;
    if (vrho_out) vrho_out[g] = vr;
    if (vsig_out) vsig_out[g] = vs;
    if (wv) {
        double ww = w[g];
        wv[g] = 0.5 * ww * vr;
        if (gga) {
            double f = 2.0 * ww * vs;
            wv[ng + g] = f * gx; wv[2 * ng + g] = f * gy; wv[3 * ng + g] = f * gz;
        }
    }
}

// Spin-polarised evaluation (UKS): rho_s[0] = density, rho_s[1..3] = its gradient.  exc[g] = e per volume;
// wv_s[0] = 0.5 w de/drho_s ; wv_s[1..3] = w (2 de/dsigma_ss grad rho_s + de/dsigma_ab grad rho_s')  (same consumer as the
// closed-shell wv: V_s = ao^T aow_s + transpose).  MGGA: dual numbers over tau_a, tau_b as well, wv_s[4] = 0.25 w de/dtau_s;
// without it the taus are not read and `gga` chooses between LDA and GGA.
template <bool MGGA>
__global__ __launch_bounds__(256) void xc_eval_spin_kernel(XcSpec X, const double *rhoa, const double *rhob, const double *taua,
                                                           const double *taub, const double *w, int64_t ng, int gga, double *exc,
                                                           double *wva, double *wvb)
{
    constexpr int NV = MGGA ? 7 : 5;
    typedef DN<NV> D;
    int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ng) return;
    const double ra = fmax(rhoa[g], 0.0), rb = fmax(rhob[g], 0.0);
    double ga[3] = {0, 0, 0}, gb[3] = {0, 0, 0};
    if (MGGA || gga)
        for (int k = 0; k < 3; k++) { ga[k] = rhoa[(k + 1) * ng + g]; gb[k] = rhob[(k + 1) * ng + g]; }
    double e = 0.0, v[NV] = {};
    if (ra + rb > 1e-10) {
        D Ra = D::var(ra, 0), Rb = D::var(rb, 1);
        D Saa = D::var(ga[0] * ga[0] + ga[1] * ga[1] + ga[2] * ga[2], 2);
        D Sab = D::var(ga[0] * gb[0] + ga[1] * gb[1] + ga[2] * gb[2], 3);
        D Sbb = D::var(gb[0] * gb[0] + gb[1] * gb[1] + gb[2] * gb[2], 4);
        D Ta(0.0), Tb(0.0);
        if constexpr (MGGA) { Ta = D::var(fmax(taua[g], 0.0), 5); Tb = D::var(fmax(taub[g], 0.0), 6); }
        D acc = xc_spin_sum<MGGA>(X, Ra, Rb, Saa, Sab, Sbb, Ta, Tb);
        e = acc.v;
        for (int k = 0; k < NV; k++) v[k] = acc.d[k];
    }
    if (exc) exc[g] = e;
    const double ww = w[g];
    wva[g] = 0.5 * ww * v[0];
    wvb[g] = 0.5 * ww * v[1];
    if (MGGA || gga)
        for (int k = 0; k < 3; k++) {
            wva[(k + 1) * ng + g] = ww * (2.0 * v[2] * ga[k] + v[3] * gb[k]);
            wvb[(k + 1) * ng + g] = ww * (2.0 * v[4] * gb[k] + v[3] * ga[k]);
        }
    if constexpr (MGGA) {
        wva[4 * ng + g] = 0.25 * ww * v[5];
        wvb[4 * ng + g] = 0.25 * ww * v[6];
    }
}

// kinds / coefs / params -> XcSpec, for every XC entry point.  `params` (may be NULL) carries each term's runtime parameter:
// the omega of XC_B88_SR, without which that term is refused.  Meta-GGA ids pass only where the caller has tau.
static int fill_xc_spec(XcSpec &X, const int32_t *kinds, const double *coefs, const double *params, int nterms, bool allow_mgga,
                        const char *who)
{
    if (nterms < 0 || nterms > 8) return fail("%s: at most 8 functional terms", who);
    X = XcSpec{};
    X.n = nterms;
    for (int i = 0; i < nterms; i++) {
        const bool mgga = kinds[i] >= XC_TPSS_X && kinds[i] <= XC_M062X_C;
        if (!xc_gga_kind(kinds[i]) && !mgga) return fail("%s: unknown functional id %d", who, kinds[i]);
        if (mgga && !allow_mgga) return fail("%s: functional id %d is a meta-GGA (needs tau: mi_xc_eval_mgga*)", who, kinds[i]);
        X.kind[i] = kinds[i]; X.coef[i] = coefs[i]; X.param[i] = params ? params[i] : 0.0;
        if (kinds[i] == XC_B88_SR && !(X.param[i] > 0.0 && std::isfinite(X.param[i])))
            return fail("%s: term %d (short-range B88) needs omega > 0 in params", who, i);
    }
    return 0;
}

// The argument check of the per-point XC entry points: -1 on an error, 0 when there is nothing to launch (ng == 0), else 1.
static int xc_entry(XcSpec &X, const int32_t *kinds, const double *coefs, const double *params, int nterms, bool allow_mgga,
                    bool null_argument, int64_t ng, const char *who)
{
    if (null_argument) return fail("%s: null argument", who);
    if (ng < 0) return fail("%s: negative number of grid points", who);
    if (fill_xc_spec(X, kinds, coefs, params, nterms, allow_mgga, who)) return -1;
    return ng > 0;
}

// ... and their launch: one thread per grid point
template <class... P, class... A> static int xc_launch(void (*kernel)(P...), int64_t ng, void *stream, A... args)
{
    hipLaunchKernelGGL(kernel, dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, (hipStream_t)stream, args...);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int mi_xc_eval_spin_p(const int32_t *kinds, const double *coefs, const double *params, int nterms, const double *d_rhoa,
                                 const double *d_rhob, const double *d_w, int64_t ng, int gga, double *d_exc, double *d_wva, double *d_wvb,
                                 void *stream)
{
    XcSpec X;
    const int go = xc_entry(X, kinds, coefs, params, nterms, false, !d_rhoa || !d_rhob || !d_w || !d_wva || !d_wvb, ng, "mi_xc_eval_spin");
    if (go <= 0) return go;
    return xc_launch(xc_eval_spin_kernel<false>, ng, stream, X, d_rhoa, d_rhob, (const double *)nullptr, (const double *)nullptr, d_w,
                     ng, gga, d_exc, d_wva, d_wvb);
}

extern "C" int mi_xc_eval_spin(const int32_t *kinds, const double *coefs, int nterms, const double *d_rhoa, const double *d_rhob,
                               const double *d_w, int64_t ng, int gga, double *d_exc, double *d_wva, double *d_wvb, void *stream)
{
    return mi_xc_eval_spin_p(kinds, coefs, nullptr, nterms, d_rhoa, d_rhob, d_w, ng, gga, d_exc, d_wva, d_wvb, stream);
}

extern "C" int mi_xc_eval_p(const int32_t *kinds, const double *coefs, const double *params, int nterms, const double *d_rho,
                            const double *d_w, int64_t ng, int gga, double *d_exc, double *d_wv, double *d_vrho, double *d_vsigma,
                            void *stream)
{
    XcSpec X;
    const int go = xc_entry(X, kinds, coefs, params, nterms, false, !d_rho || (d_wv && !d_w), ng, "mi_xc_eval");
    if (go <= 0) return go;
    return xc_launch(xc_eval_kernel, ng, stream, X, d_rho, d_w, ng, gga, d_exc, d_wv, d_vrho, d_vsigma);
}

extern "C" int mi_xc_eval(const int32_t *kinds, const double *coefs, int nterms, const double *d_rho, const double *d_w,
                          int64_t ng, int gga, double *d_exc, double *d_wv, double *d_vrho, double *d_vsigma, void *stream)
{
    return mi_xc_eval_p(kinds, coefs, nullptr, nterms, d_rho, d_w, ng, gga, d_exc, d_wv, d_vrho, d_vsigma, stream);
}

// ---- XC response (closed-shell TDDFT).  A trial density rho1 (with grad rho1) enters the linearised potential through four
// coefficients per point, coef = w {f_rr, f_rs, f_ss, v_s}:
//   s1 = 2 grad rho0 . grad rho1,  wv1[0] = 1/2 (f_rr rho1 + f_rs s1),  wv1[1..3] = 2 ((f_rs rho1 + f_ss s1) grad rho0 + v_s grad rho1)
// (w folded in), the layout of xc_eval_kernel's wv.  Singlet: the closed-shell functional's d2e/drho2, d2e/drho dsigma,
// d2e/dsigma2 and de/dsigma.  Triplet (rho_a = rho_b = rho/2 moved by +-rho1/2): the same four numbers are the derivatives of
// g(x, y, z) = e(rho/2 + x/2, rho/2 - x/2, sigma/4 + y/4 + z/4, sigma/4 - z/4, sigma/4 - y/4 + z/4) at 0 -- g_xx, g_xy, g_yy,
// g_z -- i.e. (f_aa - f_ab)/2, (f_a,saa - f_a,sbb)/4, (f_saa,saa - f_saa,sbb)/8 and v_saa/2 - v_sab/4 of the spin-polarised
// functional, which is evaluated over the three variables (x, y, z) only (10 doubles per value instead of the 21 of a full
// Hessian in five).  Points at or below the density cut-off of xc_eval_kernel / xc_eval_spin_kernel (rho <= 1e-10) get zero.
// sigma is floored at 1e-40: d2/dsigma2 of the sqrt(sigma) inside B88 is infinite at sigma = 0, where its products with
// grad rho0 vanish anyway.
template <bool TRIPLET>
__global__ __launch_bounds__(256) void xc_fxc_prep_kernel(XcSpec X, const double *rho, const double *w, int64_t ng, int gga, double *coef)
{
    int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ng) return;
    const double r = rho[g];
    double s = 1e-40;
    if (gga) {
        const double gx = rho[ng + g], gy = rho[2 * ng + g], gz = rho[3 * ng + g];
        s = fmax(gx * gx + gy * gy + gz * gz, 1e-40);
    }
    double c[4] = {0.0, 0.0, 0.0, 0.0};
    if (r > 1e-10) {
        if (!TRIPLET) {
            typedef HD<2> H;
            H acc = xc_closed_sum(X, H::var(r, 0), H::var(s, 1));
            c[0] = acc.hess(0, 0); c[1] = acc.hess(0, 1); c[2] = acc.hess(1, 1); c[3] = acc.d[1];
        } else {
            typedef HD<3> H;
            H Ra(0.5 * r), Rb(0.5 * r), Saa(0.25 * s), Sab(0.25 * s), Sbb(0.25 * s);
            Ra.d[0] = 0.5; Rb.d[0] = -0.5;
            Saa.d[1] = 0.25; Saa.d[2] = 0.25;
            Sbb.d[1] = -0.25; Sbb.d[2] = 0.25;
            Sab.d[2] = -0.25;
            H acc = xc_spin_sum(X, Ra, Rb, Saa, Sab, Sbb);
            c[0] = acc.hess(0, 0); c[1] = acc.hess(0, 1); c[2] = acc.hess(1, 1); c[3] = acc.d[2];
        }
    }
    const double ww = w[g];
    coef[g] = ww * c[0];
    if (gga) {
        coef[ng + g] = ww * c[1]; coef[2 * ng + g] = ww * c[2]; coef[3 * ng + g] = ww * c[3];
    }
}

// m trial densities rho1[m][(1|4)][ng] -> wv1[m][(1|4)][ng]; rho0 and coef read once per point for all m
__global__ __launch_bounds__(256) void xc_fxc_apply_kernel(const double *__restrict__ rho0, const double *__restrict__ coef,
                                                           const double *__restrict__ rho1, int m, int64_t ng, int gga,
                                                           double *__restrict__ wv1)
{
    int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ng) return;
    const int nc = gga ? 4 : 1;
    const double c0 = coef[g];
    if (!gga) {
        for (int j = 0; j < m; j++) wv1[(int64_t)j * ng + g] = 0.5 * c0 * rho1[(int64_t)j * ng + g];
        return;
    }
    const double c1 = coef[ng + g], c2 = coef[2 * ng + g], c3 = coef[3 * ng + g];
    const double g0x = rho0[ng + g], g0y = rho0[2 * ng + g], g0z = rho0[3 * ng + g];
    for (int j = 0; j < m; j++) {
        const double *r1 = rho1 + (int64_t)j * nc * ng;
        double *o = wv1 + (int64_t)j * nc * ng;
        const double r = r1[g], gx = r1[ng + g], gy = r1[2 * ng + g], gz = r1[3 * ng + g];
        const double s1 = 2.0 * (g0x * gx + g0y * gy + g0z * gz);
        const double t = 2.0 * (c1 * r + c2 * s1), u = 2.0 * c3;
        o[g] = 0.5 * (c0 * r + c1 * s1);
        o[ng + g] = t * g0x + u * gx;
        o[2 * ng + g] = t * g0y + u * gy;
        o[3 * ng + g] = t * g0z + u * gz;
    }
}

extern "C" int mi_xc_fxc_prep(const int32_t *kinds, const double *coefs, const double *params, int nterms, const double *d_rho,
                              const double *d_w, int64_t ng, int gga, int triplet, double *d_coef, void *stream)
{
    XcSpec X;
    const int go = xc_entry(X, kinds, coefs, params, nterms, false, !d_rho || !d_w || !d_coef, ng, "mi_xc_fxc_prep");
    if (go <= 0) return go;
    return xc_launch(triplet ? xc_fxc_prep_kernel<true> : xc_fxc_prep_kernel<false>, ng, stream, X, d_rho, d_w, ng, gga ? 1 : 0, d_coef);
}

extern "C" int mi_xc_fxc_apply(const double *d_rho0, const double *d_coef, const double *d_rho1, int m, int64_t ng, int gga,
                               double *d_wv1, void *stream)
{
    if (m < 0 || ng < 0) return fail("mi_xc_fxc_apply: negative size");
    if (m == 0 || ng == 0) return 0;
    if (!d_rho0 || !d_coef || !d_rho1 || !d_wv1) return fail("mi_xc_fxc_apply: null argument");
    hipLaunchKernelGGL(xc_fxc_apply_kernel, dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_rho0, d_coef, d_rho1,
                       m, ng, gga ? 1 : 0, d_wv1);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- meta-GGA evaluation.  Closed shell: rho[0..3] = density and gradient, tau = 1/2 sum_i |grad phi_i|^2 (all electrons);
// wv[0] = 0.5 w de/drho, wv[1..3] = 2 w de/dsigma grad rho, wv[4] = 0.25 w de/dtau  (V = vmat + vmat^T with
// vmat = ao0^T (wv0 ao0 + wv_k ao_k) + sum_k ao_k^T (wv4 ao_k)).
// The spin forms at half densities (xc_term_spin), not the closed-form functionals of xc_eval_kernel.
typedef DN<3> D3;
__global__ __launch_bounds__(256) void xc_eval_mgga_kernel(XcSpec X, const double *rho, const double *tau, const double *w, int64_t ng,
                                                           double *exc, double *wv)
{
    int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ng) return;
    const double r = rho[g], gx = rho[ng + g], gy = rho[2 * ng + g], gz = rho[3 * ng + g], t = tau[g];
    double e = 0.0, vr = 0.0, vs = 0.0, vt = 0.0;
    if (r > 1e-10) {
        D3 R = D3::var(r, 0), S = D3::var(gx * gx + gy * gy + gz * gz, 1), Tt = D3::var(fmax(t, 0.0), 2);
        D3 Rh = R * D3(0.5), S4 = S * D3(0.25), Th = Tt * D3(0.5);
        D3 acc = xc_spin_sum<true>(X, Rh, Rh, S4, S4, S4, Th, Th);
        e = acc.v; vr = acc.d[0]; vs = acc.d[1]; vt = acc.d[2];
    }
    if (exc) exc[g] = e;
    if (wv) {
        const double ww = w[g], f = 2.0 * ww * vs;
        wv[g] = 0.5 * ww * vr;
        wv[ng + g] = f * gx; wv[2 * ng + g] = f * gy; wv[3 * ng + g] = f * gz;
        wv[4 * ng + g] = 0.25 * ww * vt;
    }
}

// No term of a meta-GGA takes a runtime parameter: params = NULL, so a short-range B88 term is refused here.
extern "C" int mi_xc_eval_mgga(const int32_t *kinds, const double *coefs, int nterms, const double *d_rho, const double *d_tau,
                               const double *d_w, int64_t ng, double *d_exc, double *d_wv, void *stream)
{
    XcSpec X;
    const int go = xc_entry(X, kinds, coefs, nullptr, nterms, true, !d_rho || !d_tau || (d_wv && !d_w), ng, "mi_xc_eval_mgga");
    if (go <= 0) return go;
    return xc_launch(xc_eval_mgga_kernel, ng, stream, X, d_rho, d_tau, d_w, ng, d_exc, d_wv);
}

extern "C" int mi_xc_eval_mgga_spin(const int32_t *kinds, const double *coefs, int nterms, const double *d_rhoa, const double *d_rhob,
                                    const double *d_taua, const double *d_taub, const double *d_w, int64_t ng, double *d_exc, double *d_wva,
                                    double *d_wvb, void *stream)
{
    XcSpec X;
    const int go = xc_entry(X, kinds, coefs, nullptr, nterms, true, !d_rhoa || !d_rhob || !d_taua || !d_taub || !d_w || !d_wva || !d_wvb,
                            ng, "mi_xc_eval_mgga_spin");
    if (go <= 0) return go;
    return xc_launch(xc_eval_spin_kernel<true>, ng, stream, X, d_rhoa, d_rhob, d_taua, d_taub, d_w, ng, 1, d_exc, d_wva, d_wvb);
}

// aow[mu][g] = ao0*wv0 + sum_k ao_k*wv_k
__global__ __launch_bounds__(256) void xc_aow_kernel(const double *ao, const double *wv, int nao, int64_t ng, int gga, double *aow)
{
    int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ng) return;
    const size_t comp = (size_t)nao * ng;
    double w0 = wv[g], w1 = gga ? wv[ng + g] : 0, w2 = gga ? wv[2 * ng + g] : 0, w3 = gga ? wv[3 * ng + g] : 0;
    for (int m = blockIdx.y; m < nao; m += gridDim.y) {
        size_t o = (size_t)m * ng + g;
        double v = ao[o] * w0;
        if (gga) v += ao[comp + o] * w1 + ao[2 * comp + o] * w2 + ao[3 * comp + o] * w3;
        aow[o] = v;
    }
}

extern "C" int mi_xc_aow(mi_ctx *c, const double *d_ao, const double *d_wv, int64_t ng, int gga, double *d_aow, void *stream)
{
    if (!c) return fail("mi_xc_aow: null context");
    if (ng < 0) return fail("mi_xc_aow: negative number of grid points");
    if (ng == 0) return 0;   // nothing to write (a zero-sized grid would be a launch error)
    if (!d_ao || !d_wv || !d_aow) return fail("mi_xc_aow: null argument");
    dim3 grid((unsigned)((ng + 255) / 256), (unsigned)std::min(c->nao, 64));
    hipLaunchKernelGGL(xc_aow_kernel, grid, dim3(256), 0, (hipStream_t)stream, d_ao, d_wv, c->nao, ng, gga, d_aow);
    HIPCHK(hipGetLastError());
    return 0;
}

// =================================================================================================
// SP2 density-matrix purification helpers (row a11 without a diagonalisation): the X*X products are
// rocBLAS DGEMMs; these kernels fuse everything else so one purification step is 2 launches.
// =================================================================================================
// Gershgorin discs, one wave per row (coalesced): rows[r] = F_rr - R_r, rows[n + r] = F_rr + R_r
__global__ __launch_bounds__(256) void sp2_bounds_kernel(const double *F, int n, double *rows)
{
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= n) return;
    double s = 0.0;
    for (int c = lane; c < n; c += 64) s += fabs(F[(size_t)r * n + c]);
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) {
        double d = F[(size_t)r * n + r];
        s -= fabs(d);
        rows[r] = d - s;
        rows[n + r] = d + s;
    }
}

// X0 = (emax I - F) / (emax - emin); every block reduces the 2n disc bounds itself (cheap, no extra launch)
__global__ __launch_bounds__(256) void sp2_init_kernel(const double *F, const double *rows, int n, double *X)
{
    __shared__ double smin[256], smax[256];
    double lo = 1e300, hi = -1e300;
    for (int r = threadIdx.x; r < n; r += 256) { lo = fmin(lo, rows[r]); hi = fmax(hi, rows[n + r]); }
    smin[threadIdx.x] = lo; smax[threadIdx.x] = hi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            smin[threadIdx.x] = fmin(smin[threadIdx.x], smin[threadIdx.x + o]);
            smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + o]);
        }
        __syncthreads();
    }
    const double emin = smin[0], emax = smax[0];
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)n * n) return;
    int r = (int)(idx / n), c = (int)(idx - (size_t)r * n);
    X[idx] = ((r == c ? emax : 0.0) - F[idx]) / (emax - emin);
}

// out <- X2 if |tr X2 - N| < |2 tr X - tr X2 - N| else 2X - X2 ; traces recomputed per block (2n loads)
__global__ __launch_bounds__(256) void sp2_update_kernel(double *X, const double *X2, int n, double target, double *traces)
{
    __shared__ double s1[256], s2[256];
    double a = 0.0, b = 0.0;
    for (int r = threadIdx.x; r < n; r += 256) { a += X[(size_t)r * n + r]; b += X2[(size_t)r * n + r]; }
    s1[threadIdx.x] = a; s2[threadIdx.x] = b;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) { s1[threadIdx.x] += s1[threadIdx.x + o]; s2[threadIdx.x] += s2[threadIdx.x + o]; }
        __syncthreads();
    }
    const double tx = s1[0], tx2 = s2[0];
    const bool sq = fabs(tx2 - target) < fabs(2.0 * tx - tx2 - target);
    if (blockIdx.x == 0 && threadIdx.x == 0) { traces[0] = tx; traces[1] = tx2; }
    // the update goes to a separate buffer (after the two trace slots), so no block races with another
    // block's diagonal reads of X
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < (size_t)n * n) {
        double x = X[idx], x2 = X2[idx];
        traces[2 + idx] = sq ? x2 : 2.0 * x - x2; // out buffer follows the 2 trace slots
    }
}

extern "C" int mi_sp2_init(mi_ctx *c, const double *d_F, double *d_X, double *d_work, void *stream)
{
    if (!c || !d_F || !d_X || !d_work) return fail("mi_sp2_init: null argument");
    int n = c->nao;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sp2_bounds_kernel, dim3((n + 3) / 4), dim3(256), 0, st, d_F, n, d_work);
    hipLaunchKernelGGL(sp2_init_kernel, dim3((unsigned)(((size_t)n * n + 255) / 256)), dim3(256), 0, st, d_F, d_work, n, d_X);
    HIPCHK(hipGetLastError());
    return 0;
}

// d_out_with_traces: [2 + n*n] doubles: traces (tr X, tr X2 of the INPUT) then the updated matrix
extern "C" int mi_sp2_update(mi_ctx *c, double *d_X, const double *d_X2, double n_occ, double *d_out_with_traces, void *stream)
{
    if (!c || !d_X || !d_X2 || !d_out_with_traces) return fail("mi_sp2_update: null argument");
    int n = c->nao;
    hipLaunchKernelGGL(sp2_update_kernel, dim3((unsigned)(((size_t)n * n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_X, d_X2, n, n_occ,
                       d_out_with_traces);
    HIPCHK(hipGetLastError());
    return 0;
}

// =================================================================================================
// Analytic nuclear gradient, one-electron part (row a15):
//   g[X] += 2 sum_{mu on X, nu} [ D_mu,nu <d mu|T+V|nu> - W_mu,nu <d mu|nu> ]  (basis-function derivative)
//   g[C] -= 2 sum_{mu,nu} D_mu,nu <d mu|v_C|nu>                               (Hellmann-Feynman, via
//                                                                               translational invariance)
// One thread per ORDERED shell pair (ish, jsh); the derivative acts on the first shell.  d/dA_x of a
// primitive cartesian Gaussian = 2a (a+1_x) - a_x (a-1_x), applied inside the primitive loop.  One launch per angular class
// from the context's ordered pair list; the integral pieces are the one-electron section's (attraction_table, overlap_table, ...).
// =================================================================================================
struct Grad1eArgs : BasisDev {
    const int *pairs;    // [npair][2] ordered shell pairs of the launch's class
    int npair;
    const double *D, *W; // [nao][nao]
    double *grad;        // [natm][3]
};

template <int LA, int LB>
__global__ __launch_bounds__(64) void int1e_grad_kernel(Grad1eArgs A)
{
    constexpr int NCA = (LA + 1) * (LA + 2) / 2, NCB = (LB + 1) * (LB + 2) / 2;
    constexpr int NR = (LA + LB + 1) / 2 + 1, NI = LA + LB + 2;   // the differentiated bra reaches LA + 1
    const int pid = blockIdx.x * blockDim.x + threadIdx.x;
    if (pid >= A.npair) return;
    // grid.y = natm + 1 slices, as in int1e_kernel: y < natm: nuclear attraction of nucleus y; y == natm: overlap + kinetic
    const int vatom = (int)blockIdx.y < A.natm ? (int)blockIdx.y : -1;
    if (vatom >= 0 && A.atm[vatom * ATM_SLOTS + 0] == 0) return;
    const int ish = A.pairs[2 * pid], jsh = A.pairs[2 * pid + 1];
    const int32_t *bi = A.bas + ish * BAS_SLOTS, *bj = A.bas + jsh * BAS_SLOTS;
    const double *ra = A.env + A.atm[bi[0] * ATM_SLOTS + 1], *rb = A.env + A.atm[bj[0] * ATM_SLOTS + 1];
    const double AB[3] = {ra[0] - rb[0], ra[1] - rb[1], ra[2] - rb[2]};
    const double *ca = A.c2s + A.c2s_off[LA], *cb = A.c2s + A.c2s_off[LB];
    const int ao_i = A.shell_ao[ish], ao_j = A.shell_ao[jsh];
    double Dc[NCA * NCB];
#pragma unroll
    for (int ia = 0; ia < NCA; ia++)
#pragma unroll
        for (int ib = 0; ib < NCB; ib++) Dc[ia * NCB + ib] = density_block_to_cartesian<LA, LB>(A.D, A.nao, ao_i, ao_j, ca, cb, ia, ib);
    double gA[3] = {0.0, 0.0, 0.0};
    if (vatom >= 0) {   // nuclear attraction with the differentiated bra; the operator's own derivative by translational invariance
        const double Z = A.atm[vatom * ATM_SLOTS + 0];
        const double *C = A.env + A.atm[vatom * ATM_SLOTS + 1];
        for (int ip = 0; ip < bi[2]; ip++)
            for (int jp = 0; jp < bj[2]; jp++) {
                const PrimPair q = prim_pair(A.env, bi, bj, ip, jp, ra, rb, AB);
#pragma unroll
                for (int r = 0; r < NR; r++) {
                    double gt[3][NI][LB + 1];
                    const double f = attraction_table<LB, NI, false>(gt, q, C, 0.0, AB, NR, r, A.rys);
                    attraction_bra_gradient<LA, LB>(gA, gt, -2.0 * Z * f, q.a, Dc);
                }
            }
        for (int x = 0; x < 3; x++) atomicAdd(&A.grad[vatom * 3 + x], -gA[x]);
    } else {            // overlap and kinetic: 1-D factors S(i,j), T(i,j) for i in {a-1, a, a+1}
        double Wc[NCA * NCB];
#pragma unroll
        for (int ia = 0; ia < NCA; ia++)
#pragma unroll
            for (int ib = 0; ib < NCB; ib++) Wc[ia * NCB + ib] = density_block_to_cartesian<LA, LB>(A.W, A.nao, ao_i, ao_j, ca, cb, ia, ib);
        for (int ip = 0; ip < bi[2]; ip++)
            for (int jp = 0; jp < bj[2]; jp++) {
                const PrimPair q = prim_pair(A.env, bi, bj, ip, jp, ra, rb, AB);
                double s[3][LA + 2][LB + 3];
                overlap_table<LA, LB>(s, q);
                const double pref = q.cc * q.ex * pow(M_PI / q.p, 1.5);
#pragma unroll
                for (int ia = 0; ia < NCA; ia++)
#pragma unroll
                    for (int ib = 0; ib < NCB; ib++) {
                        double s0[3], t0[3], sd[3], td[3]; // plain and differentiated 1-D factors
#pragma unroll
                        for (int d = 0; d < 3; d++) {
                            const int i = cart_exp(LA, ia, d), j = cart_exp(LB, ib, d), im = i > 0 ? i - 1 : 0;
                            s0[d] = s[d][i][j]; t0[d] = kinetic_1d(s[d], i, j, q.b);
                            sd[d] = 2.0 * q.a * s[d][i + 1][j] - (i > 0 ? i * s[d][im][j] : 0.0);
                            td[d] = 2.0 * q.a * kinetic_1d(s[d], i + 1, j, q.b) - (i > 0 ? i * kinetic_1d(s[d], im, j, q.b) : 0.0);
                        }
                        const double dc = Dc[ia * NCB + ib], wc = Wc[ia * NCB + ib];
#pragma unroll
                        for (int x = 0; x < 3; x++) {
                            const int y = (x + 1) % 3, z = (x + 2) % 3;
                            const double dS = sd[x] * s0[y] * s0[z];
                            const double dT = td[x] * s0[y] * s0[z] + sd[x] * t0[y] * s0[z] + sd[x] * s0[y] * t0[z];
                            gA[x] += 2.0 * pref * (dc * dT - wc * dS);
                        }
                    }
            }
    }
    for (int x = 0; x < 3; x++) atomicAdd(&A.grad[bi[0] * 3 + x], gA[x]);
}

extern "C" int mi_grad_1e(mi_ctx *c, const double *d_D, const double *d_W, double *d_grad, void *stream)
{
    if (c && check_orbital_lmax(c, "mi_grad_1e")) return -1;
    if (!c || !d_D || !d_W || !d_grad) return fail("mi_grad_1e: null argument");
    HIPCHK(hipSetDevice(c->device));
    Grad1eArgs A{basis_dev(c)};
    A.D = d_D; A.W = d_W; A.grad = d_grad;
    return launch_pair_classes<true>(c, 1, "mi_grad_1e", [&](auto la, auto lb, int first, int count) {
        A.pairs = c->pair_classes[1].d_pairs + 2 * first;
        A.npair = count;
        hipLaunchKernelGGL((int1e_grad_kernel<decltype(la)::value, decltype(lb)::value>), dim3((count + 63) / 64, c->natm + 1), dim3(64), 0,
                           (hipStream_t)stream, A);
    });
}

// =================================================================================================
// Analytic nuclear gradient, two-electron part (row a15).
//
//   dE2/dR_X = 2 sum_{mu on X; nu,lam,sig} (d mu nu|lam sig) G,  G = D_mn D_ls - (hyb/4)(D_ml D_ns + D_ms D_nl)
//
// For every Schwarz-surviving canonical shell quartet the four role permutations (ij|kl),(ji|kl),(kl|ij),
// (lk|ij) are evaluated with the derivative on the FIRST shell.  d/dA of a contracted shell of angular
// momentum l is a combination of an (l+1) shell with coefficients 2*alpha*c and an (l-1) shell with
// coefficients c, so the same Rys kernel produces the two [e0|f0] blocks; `eri_grad_contract` applies
// HRR + derivative + cart->sph folded into per-pair matrices, contracts with G and adds 4*w_q*sum to
// grad[atom of the first shell].
// =================================================================================================
static void build_M_deriv(int l1, int l2, int sign, const double AB[3], const std::vector<double> &c1,
                          const std::vector<double> &c2, double *M /* [3][ns1*ns2][ne'] */)
{
    int lp = l1 + sign;
    int ns1 = 2 * l1 + 1, ns2 = 2 * l2 + 1, ne = ne_of(lp, l2);
    std::fill(M, M + (size_t)3 * ns1 * ns2 * ne, 0.0);
    int eoff[2 * LMAX + 4];
    eoff[lp] = 0;
    for (int e = lp; e < lp + l2 + 1; e++) eoff[e + 1] = eoff[e] + ncart(e);
    double pw[3][LMAX + 1];
    for (int d = 0; d < 3; d++) { pw[d][0] = 1.0; for (int k = 1; k <= LMAX; k++) pw[d][k] = pw[d][k - 1] * AB[d]; }
    int ia = 0;
    for (int ax = l1; ax >= 0; ax--)
        for (int ay = l1 - ax; ay >= 0; ay--, ia++) {
            int a[3] = {ax, ay, l1 - ax - ay};
            for (int x = 0; x < 3; x++) {
                double dcoef;
                int ap[3] = {a[0], a[1], a[2]};
                if (sign > 0) { ap[x] += 1; dcoef = 1.0; }
                else { if (a[x] == 0) continue; ap[x] -= 1; dcoef = -(double)a[x]; }
                int ib = 0;
                for (int bx = l2; bx >= 0; bx--)
                    for (int by = l2 - bx; by >= 0; by--, ib++) {
                        int bz = l2 - bx - by;
                        for (int ix = 0; ix <= bx; ix++)
                            for (int iy = 0; iy <= by; iy++)
                                for (int iz = 0; iz <= bz; iz++) {
                                    double coef = dcoef * binom(bx, ix) * binom(by, iy) * binom(bz, iz) * pw[0][bx - ix] * pw[1][by - iy] * pw[2][bz - iz];
                                    int deg = lp + ix + iy + iz;
                                    int e = eoff[deg] + cart_index(deg, ap[0] + ix, ap[1] + iy);
                                    for (int sa = 0; sa < ns1; sa++) {
                                        double v1 = c1[(size_t)ia * ns1 + sa];
                                        if (v1 == 0.0) continue;
                                        for (int sb = 0; sb < ns2; sb++) {
                                            double v2 = c2[(size_t)ib * ns2 + sb];
                                            if (v2 != 0.0) M[((size_t)x * ns1 * ns2 + sa * ns2 + sb) * ne + e] += v1 * v2 * coef;
                                        }
                                    }
                                }
                    }
            }
        }
}

// Variant records of differentiated shell pairs, for the four-centre and the density-fitted gradient alike.  Pass 1 (add_pair,
// serial and cheap) fixes the offsets of every (l+1) / (l-1) record behind what the two host buffers already hold; pass 2
// (fill, OpenMP) writes their primitive records and HRR x derivative x c2s matrices.
struct VariantRecords {
    struct Job { const ShellH *I, *J; size_t prim_off, m_off; int sign; };
    std::vector<Job> jobs;
    size_t prim_end, m_end;   // running ends of the primitive-record buffer (records) and of the matrix buffer (doubles)
    VariantRecords(size_t prim_records, size_t m_doubles) : prim_end(prim_records), m_end(m_doubles) {}
    // the two variants of the pair (I differentiated, J): out[0] = l+1, out[1] = l-1 (sh_i = -1 where I is an s shell)
    void add_pair(const ShellH &I, const ShellH &J, int s1, int s2, int ao1, int ao2, PairRec out[2])
    {
        const int np = count_prim_pairs(I, J);
        for (int sg = 0; sg < 2; sg++) {
            const int sign = sg == 0 ? +1 : -1;
            out[sg] = PairRec{-1, -1, 0, 0, 0, 0, 0, 0};
            if (I.l + sign < 0) continue;
            out[sg] = PairRec{s1, s2, ao1, ao2, (int)prim_end, np, (int)m_end, 0};
            jobs.push_back({&I, &J, prim_end, m_end, sign});
            prim_end += np;
            m_end += (size_t)3 * (2 * I.l + 1) * (2 * J.l + 1) * ne_of(I.l + sign, J.l);
        }
    }
    void fill(std::vector<double> &prim, std::vector<double> &Mbuf) const
    {
        const std::vector<std::vector<double>> c2s = c2s_tables();
#pragma omp parallel for schedule(dynamic, 64) num_threads(host_threads())
        for (size_t q = 0; q < jobs.size(); q++) {
            const Job &jb = jobs[q];
            const ShellH &I = *jb.I, &J = *jb.J;
            double AB[3] = {I.r[0] - J.r[0], I.r[1] - J.r[1], I.r[2] - J.r[2]};
            write_prim_pairs(I, J, jb.sign > 0, prim.data() + jb.prim_off * 8);
            build_M_deriv(I.l, J.l, jb.sign, AB, c2s[I.l], c2s[J.l], Mbuf.data() + jb.m_off);
        }
    }
};

// host half: sizes, primitive records and derivative matrices of every variant pair (no HIP call: may run on the helper thread)
static int grad_records_host(mi_ctx *c)
{
    std::vector<double> &prim = c->h_prim, &Mbuf = c->h_M;
    VariantRecords V(prim.size() / 8, Mbuf.size());
    for (int ci = 0; ci < NPC; ci++) {
        PairClass &P = c->pc[ci];
        for (int o = 0; o < 2; o++)
            for (int sg = 0; sg < 2; sg++) P.g_recs[o][sg].resize(P.recs.size());
        for (size_t r = 0; r < P.recs.size(); r++)
            for (int o = 0; o < 2; o++) {
                int s1 = o == 0 ? P.recs[r].sh_i : P.recs[r].sh_j, s2 = o == 0 ? P.recs[r].sh_j : P.recs[r].sh_i;
                const ShellH &I = c->shells[s1], &J = c->shells[s2];
                PairRec R[2];
                V.add_pair(I, J, s1, s2, I.ao, J.ao, R);
                if (V.m_end > (size_t)INT32_MAX) return fail("gradient transformation matrices exceed 2^31 doubles");
                for (int sg = 0; sg < 2; sg++) P.g_recs[o][sg][r] = R[sg];
            }
    }
    prim.resize(V.prim_end * 8);
    Mbuf.resize(V.m_end);
    V.fill(prim, Mbuf);
    c->grad_host_ready = true;
    return 0;
}

static int prepare_grad_records(mi_ctx *c)
{
    if (c->grad_ready) return 0;
    if (c->grad_worker.joinable()) {
        c->grad_worker.join();
        if (c->grad_host_rc) return fail("%s", c->grad_host_err.c_str());
    }
    if (!c->grad_host_ready && grad_records_host(c)) return -1;
    std::vector<double> &prim = c->h_prim, &Mbuf = c->h_M;
    for (int ci = 0; ci < NPC; ci++)
        for (int o = 0; o < 2; o++)
            for (int sg = 0; sg < 2; sg++)
                if (upload(&c->pc[ci].d_g_recs[o][sg], c->pc[ci].g_recs[o][sg])) return -1;
    if (upload(&c->d_prim, prim)) return -1;
    if (upload(&c->d_M, Mbuf)) return -1;
    c->grad_ready = true;
    return 0;
}

struct GradXfArgs {
    const PairRec *dplus, *dminus; // derivative variants of the differentiated pair (dminus may be null)
    const PairRec *ket;            // base records of the other pair
    const double *Mbuf;
    const int64_t *prefix;
    int nbra;
    int64_t t0;
    int swap, same_class;
    int ne_p, ne_m, nf, ns1, ns2, nscd, nsd;
    const double *work_p, *work_m;
    int ncomp_p, ncomp_m;
    QuartetDensity dens; // the two-particle density G (unused with DF)
    const int *shell_atom;
    double *grad;
    int inv_from_second; // translational invariance: 1: the skipped shell is dp.sh_j, 0: it is cd.sh_i
    int natm3;           // grad points to GRAD_COPIES private copies of [natm*3] (atomic contention relief)
    int64_t nbatch;      // tasks in this launch
    const TaskIdx *tasks; // non-null: (bra, ket) per task, precomputed (get_task)
    QuartetScreen scr;    // same screening as EriArgs (the Rys kernel left these quartets' blocks unwritten)
    // density fitting (mi_df_grad, template flag DF): the two-particle density is not a product of D's but a dense tensor,
    // G[(a b), (P)] = Z[a * zs_i + b * zs_j + P]  (three-index: Z3[a][b][P]; two-index: Z2[P][Q], zs_j = 0), the ket is an
    // auxiliary "pair" (P, unit function) whose atoms come from `ket_atom`, and the weight is w0 instead of 4.
    const double *Z;
    int64_t zs_i, zs_j;
    const int *ket_atom;
    double w0;
};
#define GRAD_COPIES 4096

// GSZ = lanes per quartet: 16 (four quartets per wave, small angular classes) or 64 (256 = four waves sharing one
// quartet's LDS blocks is supported by the code but was measured slower and is not launched).
template <int GSZ, bool MFMA, bool DF = false, GradTerms TERMS = GradTerms::PLAIN>
__global__ __launch_bounds__(GSZ > 64 ? GSZ : 64) void eri_grad_contract(GradXfArgs A)
{
    // sum_{x-independent part first}:  g[x] = sum_{r,e} M^x[r][e] * Z[r][e],  Z[r][e] = sum_f E0[e][f] Y[r][f],
    // Y[r][f] = sum_c G[r][c] Mcd[c][f]  -- contracting the two-particle density FIRST makes the work
    // independent of the derivative direction (3x fewer flops than forming the derivative integrals).
    extern __shared__ double lds_all[];
    constexpr int QPW = GSZ >= 64 ? 1 : 64 / GSZ;
    constexpr int NW = GSZ >= 64 ? GSZ / 64 : 1;
    const int wl = threadIdx.x & 63, wave = threadIdx.x >> 6; // lane within the wave / wave within the workgroup (MFMA tiles)
    const int grp = threadIdx.x / GSZ, lane = threadIdx.x % GSZ;
    const int64_t tl = (int64_t)blockIdx.x * QPW + grp; // task index inside this batch
    const bool in_batch = tl < A.nbatch;
    const bool has_m = A.dminus != nullptr && A.ne_m > 0;
    const int nsab = A.ns1 * A.ns2, nf = A.nf;
    const size_t region = (size_t)A.ne_p * nf + (has_m ? (size_t)A.ne_m * nf : 0) + (size_t)nsab * A.nscd + (size_t)nsab * nf;
    double *lds = lds_all + (size_t)grp * region;
    double *E0p = lds;                                        // [ne_p][nf]
    double *E0m = E0p + (size_t)A.ne_p * nf;                  // [ne_m][nf]
    double *G = E0m + (has_m ? (size_t)A.ne_m * nf : 0);      // [nsab][nscd]
    double *Y = G + (size_t)nsab * A.nscd;                    // [nsab][nf]
    int ib = 0, ik = 0;
    if (in_batch) get_task(A.tasks, A.prefix, A.nbra, A.t0 + tl, ib, ik);
    const bool same_pair = A.same_class && ib == ik;
    if (A.swap) { int t_ = ib; ib = ik; ik = t_; }
    const PairRec dp = A.dplus[ib], cd = A.ket[ik];
    const bool live = in_batch && !A.scr.negligible(ib, ik, dp.sh_i, dp.sh_j, cd.sh_i, cd.sh_j);
    int m_off_m = 0;
    // the first E0PRE x GSZ elements of the plus block travel through registers: their loads are issued here and land in LDS only
    // after the Y product, so the HBM round trip of the hand-over block overlaps the G gather and the first matrix product
    constexpr int E0PRE = (GSZ >= 64 && MFMA) ? 8 : 0;
    double pre[E0PRE > 0 ? E0PRE : 1];
    const int n_e0p = A.ne_p * nf;
    if (live) {
        const double *gp = A.work_p + (size_t)tl * A.ncomp_p;
        if (E0PRE > 0) {
#pragma unroll
            for (int q = 0; q < E0PRE; q++) { const int c = lane + q * GSZ; pre[q] = c < n_e0p ? gp[c] : 0.0; }
        }
        for (int c = lane + E0PRE * GSZ; c < n_e0p; c += GSZ) E0p[c] = gp[c];
        if (has_m) {
            m_off_m = A.dminus[ib].m_off;
            const double *gm = A.work_m + (size_t)tl * A.ncomp_m;
            for (int c = lane; c < A.ne_m * nf; c += GSZ) E0m[c] = gm[c];
        }
        for (int o = lane; o < nsab * A.nscd; o += GSZ) {
            int r = o / A.nscd, c = o - r * A.nscd;
            int sa = r / A.ns2, sb = r - sa * A.ns2, sc = c / A.nsd, sd = c - sc * A.nsd;
            int i = dp.ao_i + sa, j = dp.ao_j + sb, k = cd.ao_i + sc, l = cd.ao_j + sd;
            G[o] = DF ? A.Z[(int64_t)i * A.zs_i + (int64_t)j * A.zs_j + k] : A.dens.template element<TERMS>(i, j, k, l);
        }
    }
    __syncthreads();
    // the three small matrix products run on the FP64 MFMA pipe when the whole wave works on one quartet and the
    // 16x16x4 padding does not eat the gain (wave-uniform decisions); otherwise plain per-lane dot products
    if (live) {
        const double *Mcd = A.Mbuf + cd.m_off;
        if (MFMA && GSZ >= 64 && mfma_worthwhile(nsab, nf, A.nscd)) {
            int tile = 0;
            for (int m0 = 0; m0 < nsab; m0 += 16)
                for (int n0 = 0; n0 < nf; n0 += 16) {
                    if ((tile++) % NW != wave) continue;
                    d4_t y = wave_mfma_tile(G, A.nscd, 1, nsab, Mcd, nf, 1, nf, A.nscd, m0, n0, wl);
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        int r = m0 + (wl >> 4) + 4 * q, f = n0 + (wl & 15);
                        if (r < nsab && f < nf) Y[r * nf + f] = y[q];
                    }
                }
        } else {
            for (int o = lane; o < nsab * nf; o += GSZ) {
                int r = o / nf, f = o - r * nf;
                double s = 0.0;
                for (int c = 0; c < A.nscd; c++) s += G[r * A.nscd + c] * Mcd[c * nf + f];
                Y[o] = s;
            }
        }
    }
    if (E0PRE > 0 && live) {
#pragma unroll
        for (int q = 0; q < E0PRE; q++) { const int c = lane + q * GSZ; if (c < n_e0p) E0p[c] = pre[q]; }
    }
    __syncthreads();
    double acc[3] = {0.0, 0.0, 0.0};
    if (live) {
        for (int var = 0; var < (has_m ? 2 : 1); var++) {
            const double *Mx = A.Mbuf + (var == 0 ? dp.m_off : m_off_m);
            const double *E0 = var == 0 ? E0p : E0m;
            const int ne = var == 0 ? A.ne_p : A.ne_m;
            const size_t xs = (size_t)nsab * ne;
            if (MFMA && GSZ >= 64 && mfma_worthwhile(nsab, ne, nf)) {
                int tile = 0;
                for (int m0 = 0; m0 < nsab; m0 += 16)
                    for (int n0 = 0; n0 < ne; n0 += 16) {
                        if ((tile++) % NW != wave) continue;
                        d4_t z = wave_mfma_tile(Y, nf, 1, nsab, E0, 1, nf, ne, nf, m0, n0, wl); // Z[r][e] = sum_f Y[r][f] E0[e][f]
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            int r = m0 + (wl >> 4) + 4 * q, e = n0 + (wl & 15);
                            if (r < nsab && e < ne) {
                                size_t o = (size_t)r * ne + e;
                                acc[0] += Mx[o] * z[q]; acc[1] += Mx[xs + o] * z[q]; acc[2] += Mx[2 * xs + o] * z[q];
                            }
                        }
                    }
            } else {
                for (int o = lane; o < nsab * ne; o += GSZ) {
                    int r = o / ne, e = o - r * ne;
                    double z = 0.0;
                    for (int f = 0; f < nf; f++) z += E0[e * nf + f] * Y[r * nf + f];
                    acc[0] += Mx[o] * z; acc[1] += Mx[xs + o] * z; acc[2] += Mx[2 * xs + o] * z;
                }
            }
        }
    }
    double w = DF ? A.w0 : 4.0;
    if (dp.sh_i == dp.sh_j) w *= 0.5;
    if (!DF && cd.sh_i == cd.sh_j) w *= 0.5;
    if (same_pair) w *= 0.5;
    for (int x = 0; x < 3; x++) {
        double v = acc[x];
        for (int o = (GSZ < 64 ? GSZ : 64) / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (live && (lane & ((GSZ < 64 ? GSZ : 64) - 1)) == 0) { // one partial sum per wave (per 16-lane group for GSZ = 16)
            double *gc = A.grad + (size_t)((blockIdx.x * QPW + grp) & (GRAD_COPIES - 1)) * A.natm3;
            atomicAdd(&gc[A.shell_atom[dp.sh_i] * 3 + x], w * v);
            // the skipped permutation (derivative on the first shell of the bra pair P) by invariance; density fitting:
            // the auxiliary centre takes minus the force on the differentiated orbital (or auxiliary) shell
            const int other = DF ? A.ket_atom[cd.sh_i] : A.shell_atom[A.inv_from_second ? dp.sh_j : cd.sh_i];
            atomicAdd(&gc[other * 3 + x], -w * v);
        }
    }
}

// =================================================================================================
// Derivative ERIs contracted with the two-particle density, MID / HIGH classes, "row" kernel (round 3).
//
// One wave per (live quartet, permutation), NOTHING handed over: lane e owns ROW e of the contracted [e0|f0] blocks of both
// derivative variants (rows 0 .. ne_p-1: the (l1+1, l2) block, rows ne_p .. ne_p+ne_m-1: the (l1-1, l2) block; ROWS rows per
// lane) and keeps its NF = ne(LC, LD) elements in REGISTERS; the other pair (LC, LD) is a template parameter, so the NF
// products of a row per primitive quartet and root are straight-line code over 3 (LC+LD+1) table values the lane reads from
// LDS once.  Roots, weights and the 2-D recurrence tables come from the phase functions of eri_rys_kernel (rys_phase_roots,
// rys_phase_tables; runtime l1, l2, the other pair's degree a constant); the (l1-1) rows share them -- same Gaussian product, the factor K-/K+ = 1 / (2 alpha) is applied per primitive pair.
// The gradient is LINEAR in the block, so the row is contracted where it lives:
//     Yk[c]  = sum_f E0[e][f] Mcd[c][f]                       (ket HRR + cart->sph, matrix in LDS)
//     t_r    = sum_c Yk[c] G[r][c]                            (two-particle density block in LDS)
//     g[x]  += Mx[x][r][e] t_r                                (row e of the derivative x HRR x c2s matrices, adjoint use)
// and the wave sums g over its lanes.  Against the Rys -> hand-over -> eri_grad_contract pipeline this drops both hand-over
// buffers (written and re-read once per variant), two of the three launches and their task decodes, all barriers outside the
// Rys phases, and the Z product; every table value is read from LDS once per row instead of three per component.
// =================================================================================================
template <int LC, int LD>
struct FTab {
    static constexpr int NF = c_ne(LC, LD);
    int fx[NF], fy[NF], fz[NF];
    constexpr FTab() : fx{}, fy{}, fz{}
    {
        int n = 0;
        for (int f = LC; f <= LC + LD; f++)
            for (int a = f; a >= 0; a--)
                for (int b = f - a; b >= 0; b--) { fx[n] = a; fy[n] = b; fz[n] = f - a - b; n++; }
    }
};

// LDS doubles of a quartet behind its Rys block (RysLds): K- / K+ per primitive quartet of a batch, the ket matrix, the density block
__host__ __device__ inline size_t grad_rows_lds_extra(int PB, int nscd, int nf, int nsab) { return (size_t)PB + (size_t)nscd * nf + (size_t)nsab * nscd; }

struct GradRowsArgs {
    const PairRec *dplus, *dminus, *ket;
    const double *prim, *Mbuf;
    const TaskIdx *tasks;
    const int64_t *prefix;
    int nbra;
    int64_t t0, ntask;
    int swap, same_class;
    int nmax, nroots, tsz, PB;          // Rys set-up of the (l1+1, l2 | lc, ld) variant
    int ne_p, ne_m, nsab, ns2;
    const uint32_t *comp_p, *comp_m;    // component tables of the two variants (row bases: entry e * NF)
    RysDev rys;
    QuartetDensity dens;
    const int *shell_atom;
    double *grad;
    int natm3, inv_from_second;
    QuartetScreen scr;
};

// GSZ lanes per quartet (64 / GSZ quartets per wave): the Rys phases keep 2 n .. 3 n lanes per primitive quartet busy and the
// rows of the low bra classes fill a fraction of a wave, so the small classes run two or four latency chains side by side.
template <int LC, int LD, int ROWS, int GSZ, GradTerms TERMS = GradTerms::PLAIN>
__global__ __launch_bounds__(64) void eri_grad_rows_kernel(GradRowsArgs A)
{
    constexpr int NF = c_ne(LC, LD), MMAX = LC + LD, M1 = MMAX + 1;
    constexpr int NSC = 2 * LC + 1, NSD = 2 * LD + 1, NSCD = NSC * NSD;
    constexpr int QPW = 64 / GSZ;
    constexpr FTab<LC, LD> FT{};
    extern __shared__ double lds_all[];
    const int grp = QPW == 1 ? 0 : threadIdx.x / GSZ, lane = QPW == 1 ? threadIdx.x : threadIdx.x % GSZ;
    const int64_t tl = (int64_t)blockIdx.x * QPW + grp;
    bool live = tl < A.ntask;
    int ib, ik;
    get_task(A.tasks, A.prefix, A.nbra, A.t0 + (live ? tl : 0), ib, ik);
    const bool same_pair = A.same_class && ib == ik;
    if (A.swap) { int t_ = ib; ib = ik; ik = t_; }
    const bool has_m = A.ne_m > 0;
    const PairRec dp = A.dplus[ib], cd = A.ket[ik];
    if (live && A.scr.negligible(ib, ik, dp.sh_i, dp.sh_j, cd.sh_i, cd.sh_j))
        live = false;
    if (QPW == 1 && !live) return;
    int m_prim = dp.prim_off, m_off_m = 0;
    if (has_m) { const PairRec dm = A.dminus[ib]; m_prim = dm.prim_off; m_off_m = dm.m_off; }
    const int n = A.nroots, tsz = A.tsz, PB = A.PB, nsab = A.nsab;
    const RysLds L{PB, n, tsz};
    double *T0 = lds_all + (size_t)grp * (L.doubles() + grad_rows_lds_extra(PB, NSCD, NF, nsab));   // [PB n][3][tsz], then rw [PB][2 n]
    double *rw = T0 + L.rw();
    double *rho = T0 + L.doubles();                        // [PB]   K- / K+ of the bra primitive pair
    double *McdL = rho + PB;                               // [NSCD][NF]
    double *G = McdL + NSCD * NF;                          // [nsab][NSCD]
    // ket matrix and two-particle density block (used after the Rys loop: its barriers order these writes)
    if (live) {
        const double *Mcd = A.Mbuf + cd.m_off;
        for (int q = lane; q < NSCD * NF; q += GSZ) McdL[q] = Mcd[q];
        const int ns2 = A.ns2;
        for (int o = lane; o < nsab * NSCD; o += GSZ) {      // G[r][c], r = (sa, sb) of the differentiated pair, c = (sc, sd) of the other
            const int r = o / NSCD, c = o - r * NSCD;
            const int sa = r / ns2, sb = r - sa * ns2, sc = c / NSD, sd = c - sc * NSD;
            G[o] = A.dens.template element<TERMS>(dp.ao_i + sa, dp.ao_j + sb, cd.ao_i + sc, cd.ao_j + sd);
        }
    }
    const int ne = A.ne_p + A.ne_m;
    int bx[ROWS], by[ROWS], bz[ROWS];
    bool valid[ROWS], minus[ROWS];
#pragma unroll
    for (int rr = 0; rr < ROWS; rr++) {
        const int e = lane + GSZ * rr;
        valid[rr] = live && e < ne;
        minus[rr] = e >= A.ne_p;
        uint32_t w = 0;
        if (valid[rr]) w = minus[rr] ? A.comp_m[(size_t)(e - A.ne_p) * NF] : A.comp_p[(size_t)e * NF];
        bx[rr] = (int)(w & 1023u) - LC; by[rr] = (int)((w >> 10) & 1023u); bz[rr] = (int)((w >> 20) & 1023u);
    }
    double acc[ROWS][NF];
#pragma unroll
    for (int rr = 0; rr < ROWS; rr++)
#pragma unroll
        for (int f = 0; f < NF; f++) acc[rr][f] = 0.0;
    const int ncd = cd.nprim, nPQ = live ? dp.nprim * ncd : 0;
    int nPQ_all = nPQ;   // uniform trip count over the quartets sharing this wave (the barriers sit in the loop)
    if (QPW > 1)
        for (int o = GSZ; o < 64; o <<= 1) nPQ_all = max(nPQ_all, __shfl_xor(nPQ_all, o));
    const double *prim_b = A.prim + (size_t)dp.prim_off * 8, *prim_k = A.prim + (size_t)cd.prim_off * 8;
    const double *prim_m = A.prim + (size_t)m_prim * 8;
    for (int pq0 = 0; pq0 < nPQ_all; pq0 += PB) {
        const int npq = max(0, min(PB, nPQ - pq0));
        rys_phase_roots<GSZ, false>(A.rys, 0.0, n, prim_b, prim_k, ncd, pq0, npq, lane, rw);
        if (has_m)
            for (int idx = lane; idx < npq; idx += GSZ) {       // K- / K+ of the primitive pairs of this batch
                const int ip = (pq0 + idx) / ncd;
                rho[idx] = prim_m[(size_t)ip * 8 + 7] / prim_b[(size_t)ip * 8 + 7];
            }
        __syncthreads();
        rys_phase_tables<GSZ, false>(n, A.nmax, MMAX, tsz, prim_b, prim_k, ncd, pq0, npq, lane, rw, T0);
        __syncthreads();
        const int nslot = npq * n;
        for (int s_ = 0; s_ < nslot; s_++) {
            const double *Tx = T0 + (size_t)s_ * 3 * tsz, *Ty = Tx + tsz, *Tz = Ty + tsz;
            const double rs = has_m ? rho[s_ / n] : 0.0;
#pragma unroll
            for (int rr = 0; rr < ROWS; rr++) {
                if (!valid[rr]) continue;
                double x[M1], y[M1], z[M1];
                const double sc = minus[rr] ? rs : 1.0;
#pragma unroll
                for (int m = 0; m < M1; m++) { x[m] = Tx[bx[rr] + m]; y[m] = Ty[by[rr] + m]; z[m] = Tz[bz[rr] + m] * sc; }
#pragma unroll
                for (int f = 0; f < NF; f++) acc[rr][f] = fma(x[FT.fx[f]] * y[FT.fy[f]], z[FT.fz[f]], acc[rr][f]);
            }
        }
        __syncthreads();
    }
    double g[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int rr = 0; rr < ROWS; rr++) {
        if (!valid[rr]) continue;
        double Yk[NSCD];
#pragma unroll
        for (int c = 0; c < NSCD; c++) {
            double s = 0.0;
#pragma unroll
            for (int f = 0; f < NF; f++) s = fma(acc[rr][f], McdL[c * NF + f], s);
            Yk[c] = s;
        }
        const int e = lane + GSZ * rr;
        const int nev = minus[rr] ? A.ne_m : A.ne_p, el = minus[rr] ? e - A.ne_p : e;
        const double *Mx = A.Mbuf + (minus[rr] ? m_off_m : dp.m_off) + el;
        const size_t xs = (size_t)nsab * nev;
        // the derivative-matrix elements of four r go out together (they depend on nothing computed here): one round trip per
        // four rows of G instead of one per row
        for (int r0 = 0; r0 < nsab; r0 += 4) {
            double mx[4][3];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const size_t o = (size_t)min(r0 + u, nsab - 1) * nev;
                mx[u][0] = Mx[o]; mx[u][1] = Mx[xs + o]; mx[u][2] = Mx[2 * xs + o];
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (r0 + u >= nsab) break;
                double t = 0.0;
#pragma unroll
                for (int c = 0; c < NSCD; c++) t = fma(Yk[c], G[(r0 + u) * NSCD + c], t);
                g[0] = fma(mx[u][0], t, g[0]); g[1] = fma(mx[u][1], t, g[1]); g[2] = fma(mx[u][2], t, g[2]);
            }
        }
    }
    double w = 4.0;
    if (dp.sh_i == dp.sh_j) w *= 0.5;
    if (cd.sh_i == cd.sh_j) w *= 0.5;
    if (same_pair) w *= 0.5;
#pragma unroll
    for (int x = 0; x < 3; x++) {
        double v = g[x];
        for (int o = GSZ / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (live && lane == 0) {
            double *gc = A.grad + (size_t)((blockIdx.x * QPW + grp) & (GRAD_COPIES - 1)) * A.natm3;
            atomicAdd(&gc[A.shell_atom[dp.sh_i] * 3 + x], w * v);
            atomicAdd(&gc[A.shell_atom[A.inv_from_second ? dp.sh_j : cd.sh_i] * 3 + x], -w * v);
        }
    }
}

// rows per lane and lanes per quartet by the number of rows ne of the two derivative blocks:
//   ne <= 64: (2, 32), two quartets per wave   ne <= 128: (2, 64)   ne <= 192: (3, 64)
// Measured on one box (ibuprofen/def2-TZVP, grad_dtol 1e-10, whole two-electron gradient): pipeline only 0.535 s; row kernel for
// ne > 64 only 0.504; for ne >= 33 0.495 (one quartet per wave there: 0.502); for ne >= 20 0.492; four quartets per wave
// (16 lanes) for ne <= 32: 0.518 -- the small blocks stay on the hand-over pipeline / thread-per-quartet kernels.
struct RowsGeom { int rows, gsz; };
static RowsGeom rows_geometry(int ne)
{
    if (g_rows_g32 && ne <= 64) return {2, 32};
    if (ne <= 64) return {1, 64};
    if (ne <= 128) return {2, 64};
    if (ne <= 192) return {3, 64};
    return {0, 0};
}
template <int LC, int LD, int ROWS, int GSZ, GradTerms TERMS>
static int launch_grad_rows_g(const GradRowsArgs &R, size_t shm_per_quartet, hipStream_t st)
{
    constexpr int QPW = 64 / GSZ;
    const size_t shm = shm_per_quartet * QPW;
    if (shm > 160 * 1024) return 0;
    if (shm > 64 * 1024)
        HIPCHK(hipFuncSetAttribute((const void *)eri_grad_rows_kernel<LC, LD, ROWS, GSZ, TERMS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
    hipLaunchKernelGGL((eri_grad_rows_kernel<LC, LD, ROWS, GSZ, TERMS>), dim3((unsigned)((R.ntask + QPW - 1) / QPW)), dim3(64), shm, st, R);
    HIPCHK(hipGetLastError());
    return 1;
}
template <int LC, int LD>
static int launch_grad_rows_t(RowsGeom gm, const GradRowsArgs &R, size_t shm_q, hipStream_t st)
{
    return with_grad_terms(R.dens, [&](auto terms) {
        constexpr GradTerms T = decltype(terms)::value;
        if (gm.rows == 2 && gm.gsz == 32) return launch_grad_rows_g<LC, LD, 2, 32, T>(R, shm_q, st);
        if (gm.rows == 1 && gm.gsz == 64) return launch_grad_rows_g<LC, LD, 1, 64, T>(R, shm_q, st);
        if (gm.rows == 2 && gm.gsz == 64) return launch_grad_rows_g<LC, LD, 2, 64, T>(R, shm_q, st);
        if (gm.rows == 3 && gm.gsz == 64) return launch_grad_rows_g<LC, LD, 3, 64, T>(R, shm_q, st);
        return 0;
    });
}
// 1: launched, 0: no row kernel for this (other pair, number of rows), -1: error.  dry: only answers the question.
static int launch_grad_rows(int lc, int ld, int ne, const GradRowsArgs &R, size_t shm_q, hipStream_t st, bool dry = false)
{
    const RowsGeom gm = rows_geometry(ne);
    if (gm.rows == 0) return 0;
#define ROWS_CASE(a, b) if (lc == a && ld == b) return dry ? 1 : launch_grad_rows_t<a, b>(gm, R, shm_q, st)
    ROWS_CASE(0, 0); ROWS_CASE(1, 0); ROWS_CASE(1, 1); ROWS_CASE(2, 0); ROWS_CASE(2, 1); ROWS_CASE(2, 2); ROWS_CASE(3, 0); ROWS_CASE(3, 1);
#undef ROWS_CASE
    return 0;
}

// =================================================================================================
// Derivative ERIs contracted with the two-particle density, LOW angular classes: one THREAD per (canonical quartet, role
// permutation), everything in registers (the gradient counterpart of eri_tpq_kernel; round 1 spent 1.6 of the 1.9 s of the
// ibuprofen/def2-TZVP gradient in the wave-per-quartet path of these classes).
//   d/dA_x (a b| = 2 alpha (a+1_x b| - a_x (a-1_x b|: the primitive loop accumulates the [e0|f0] blocks of the (L1+1) shell
//   (coefficients 2 alpha c, folded into the "plus" pair record) and of the (L1-1) shell side by side (same roots, same 2-D
//   recurrence tables); the ket is transformed first, then for each ket component the bra goes HRR -> derivative -> cart->sph
//   and is contracted at once with G = D_ab D_cd - hyb/4 (D_ac D_bd + D_ad D_bc) (+ spin term): no derivative block is stored.
// L1 = differentiated shell, L2 = its partner (either order), (LC >= LD) the other pair.
// =================================================================================================
// NOT folded onto QuartetDensity / QuartetScreen: this kernel keeps the fields, the screening test and the element formula in its
// own text (and two template booleans for GradTerms).  Its larger classes sit at the 512-register limit, and every folded form
// tried -- embedded structs in three member orders, by-value copies, forced inlining, a static element() on hoisted locals --
// moved VGPRs or scratch in a third of the plain classes and slowed the plain gradient by 0.6 %; with this text the compiler's
// resource figures are the unfolded ones.  The formula below must stay equal to QuartetDensity::element.
struct TpqGradArgs {
    const PairRec *dplus, *dminus, *ket;
    const double *prim;
    const int64_t *prefix;
    int nbra;
    int64_t t0, ntask;
    int swap, same_class;
    const double *c2s;
    int c2s_off[LMAX + 2];
    RysDev rys;
    const double *shell_xyz;
    const double *D, *Dm;     // padded total / spin density
    int ld;
    double hyb;
    const int *shell_atom;
    double *grad;             // GRAD_COPIES private copies of [natm3]
    int natm3, inv_from_second;
    const double *q_bra, *q_ket, *dmax;
    const double *qmax;                 // pair mode of the gradient: see quartet_density_bound (nullptr otherwise)
    const double *xmax;                 // exchange-pair mode of the gradient: see quartet_density_bound (nullptr otherwise)
    int nbas_d;
    double dtol;
    const TaskIdx *tasks;     // non-null: the compacted list of live quartets (already screened: dmax is null then)
    PairTerm pt;              // pair mode (template flag PAIRS)
    PairTerm xt;              // exchange-pair mode (template flag XPAIRS)
};

template <int L1, int L2, int LC, int LD, bool PAIRS = false, bool XPAIRS = false>
__global__ __launch_bounds__(TPQ_BLOCK) void eri_tpq_grad_kernel(TpqGradArgs A)
{
    constexpr bool HASM = L1 > 0;
    constexpr int LP = L1 + 1, LM = HASM ? L1 - 1 : 0;
    constexpr int NR = (LP + L2 + LC + LD) / 2 + 1;
    constexpr int NMAX = LP + L2, MMAX = LC + LD;
    constexpr int NEP = c_ne(LP, L2), NEM = HASM ? c_ne(LM, L2) : 0, NF = c_ne(LC, LD);
    constexpr int NS1 = 2 * L1 + 1, NS2 = 2 * L2 + 1, NSC = 2 * LC + 1, NSD = 2 * LD + 1, NSCD = NSC * NSD;
    constexpr int NK1 = c_ncart(L1), NK2 = c_ncart(L2), NCP = c_ncart(LP), NCM = HASM ? c_ncart(LM) : 1;
    extern __shared__ double cheb[];
    const int nint = A.rys.nint[NR];
    {
        const int ntab = nint * 2 * NR * (RYS_DEG + 1);
        const double *src = A.rys.cheb + A.rys.off[NR];
        for (int q = threadIdx.x; q < ntab; q += TPQ_BLOCK) cheb[q] = src[q];
    }
    __syncthreads();
    const int64_t tl = (int64_t)blockIdx.x * TPQ_BLOCK + threadIdx.x;
    bool live = tl < A.ntask;
    int ib = 0, ik = 0;
    if (live) get_task(A.tasks, A.prefix, A.nbra, A.t0 + tl, ib, ik);
    const bool same_pair = A.same_class && ib == ik;
    if (A.swap) { int t_ = ib; ib = ik; ik = t_; }
    const PairRec dp = A.dplus[ib], cd = A.ket[ik];
    if (live && A.dmax && A.q_bra[ib] * A.q_ket[ik] * quartet_density_bound(A.dmax, A.nbas_d, dp.sh_i, dp.sh_j, cd.sh_i, cd.sh_j, A.hyb, A.qmax, A.xmax) < A.dtol)
        live = false;
    double force[3] = {0.0, 0.0, 0.0};
    if (live) {
        int mprim_off = 0;
        if (HASM) mprim_off = A.dminus[ib].prim_off;
        double accp[NEP * NF], accm[(HASM ? NEM : 1) * NF];
#pragma unroll
        for (int q = 0; q < NEP * NF; q++) accp[q] = 0.0;
#pragma unroll
        for (int q = 0; q < (HASM ? NEM : 1) * NF; q++) accm[q] = 0.0;
        for (int ip = 0; ip < dp.nprim; ip++) {
            const double *b = A.prim + (size_t)(dp.prim_off + ip) * 8;
            const double p = b[0], Px = b[1], Py = b[2], Pz = b[3], Kp = b[7];
            const double Km = HASM ? A.prim[(size_t)(mprim_off + ip) * 8 + 7] : 0.0;
            const double PA[3] = {b[4], b[5], b[6]};
            for (int jp = 0; jp < cd.nprim; jp++) {
                const double *kk = A.prim + (size_t)(cd.prim_off + jp) * 8;
                const double q = kk[0];
                const double PQ[3] = {Px - kk[1], Py - kk[2], Pz - kk[3]};
                const double QC[3] = {kk[4], kk[5], kk[6]};
                const double pq1 = 1.0 / (p + q);
                const double x = p * q * pq1 * (PQ[0] * PQ[0] + PQ[1] * PQ[1] + PQ[2] * PQ[2]);
                const double pref = kk[7] * 34.986836655249725 /* 2 pi^2.5 */ * pq1 * sqrt(p + q) / (p * q);
                double u[NR], w[NR];
                if (x < nint * RYS_H) {
                    int iv = (int)(x * (1.0 / RYS_H));
                    if (iv >= nint) iv = nint - 1;
                    const double sx = (x - (iv * RYS_H + 0.5 * RYS_H)) * (2.0 / RYS_H), s2 = 2.0 * sx;
                    const double *cb = cheb + (size_t)iv * 2 * NR * (RYS_DEG + 1);
#pragma unroll
                    for (int f = 0; f < 2 * NR; f++) {
                        const double *cc = cb + f * (RYS_DEG + 1);
                        double b1 = 0.0, b2 = 0.0;
#pragma unroll
                        for (int kq = RYS_DEG; kq >= 1; kq--) {
                            double tq = s2 * b1 - b2 + cc[kq];
                            b2 = b1;
                            b1 = tq;
                        }
                        const double val = sx * b1 - b2 + cc[0];
                        if (f < NR) u[f] = val; else w[f - NR] = val;
                    }
                } else {
                    const double rx = 1.0 / x, rsx = rsqrt(x);
#pragma unroll
                    for (int f = 0; f < NR; f++) { u[f] = A.rys.herm_r[NR * RYS_NMAX + f] * rx; w[f] = A.rys.herm_w[NR * RYS_NMAX + f] * rsx; }
                }
#pragma unroll
                for (int r = 0; r < NR; r++) {
                    const double ur = u[r];
                    const double b00 = 0.5 * ur * pq1, b10 = 0.5 / p * (1.0 - ur * q * pq1), b01 = 0.5 / q * (1.0 - ur * p * pq1);
                    double T[3][NMAX + 1][MMAX + 1];
#pragma unroll
                    for (int d = 0; d < 3; d++) {
                        const double c00 = PA[d] - ur * q * pq1 * PQ[d], c01 = QC[d] + ur * p * pq1 * PQ[d];
                        T[d][0][0] = d == 2 ? w[r] * pref : 1.0;
#pragma unroll
                        for (int n = 0; n < NMAX; n++) T[d][n + 1][0] = c00 * T[d][n][0] + (n > 0 ? n * b10 * T[d][n - 1][0] : 0.0);
#pragma unroll
                        for (int m = 0; m < MMAX; m++)
#pragma unroll
                            for (int n = 0; n <= NMAX; n++) {
                                double v = c01 * T[d][n][m];
                                if (m > 0) v = fma(m * b01, T[d][n][m - 1], v);
                                if (n > 0) v = fma(n * b00, T[d][n - 1][m], v);
                                T[d][n][m + 1] = v;
                            }
                    }
#pragma unroll
                    for (int df = LC; df <= LC + LD; df++)
#pragma unroll
                        for (int fx = df; fx >= 0; fx--)
#pragma unroll
                            for (int fy = df - fx; fy >= 0; fy--) {
                                const int fz = df - fx - fy, jf = c_eoff(LC, df) + c_cidx(df, fx, fy);
                                // plus block: degrees LP .. LP + L2
#pragma unroll
                                for (int de = LP; de <= LP + L2; de++)
#pragma unroll
                                    for (int ex = de; ex >= 0; ex--)
#pragma unroll
                                        for (int ey = de - ex; ey >= 0; ey--) {
                                            const int ez = de - ex - ey, ie = c_eoff(LP, de) + c_cidx(de, ex, ey);
                                            accp[ie * NF + jf] = fma(Kp * T[0][ex][fx] * T[1][ey][fy], T[2][ez][fz], accp[ie * NF + jf]);
                                        }
                                if (HASM) {
#pragma unroll
                                    for (int de = LM; de <= LM + L2; de++)
#pragma unroll
                                        for (int ex = de; ex >= 0; ex--)
#pragma unroll
                                            for (int ey = de - ex; ey >= 0; ey--) {
                                                const int ez = de - ex - ey, ie = c_eoff(LM, de) + c_cidx(de, ex, ey);
                                                accm[ie * NF + jf] = fma(Km * T[0][ex][fx] * T[1][ey][fy], T[2][ez][fz], accm[ie * NF + jf]);
                                            }
                                }
                            }
                }
            }
        }
        // ---- ket: HRR + cart->sph on the f index of both blocks
        const MI_CONST_AS double *c2s = as_const(A.c2s);
        double ABv[3], CDv[3];
#pragma unroll
        for (int d = 0; d < 3; d++) {
            ABv[d] = A.shell_xyz[3 * dp.sh_i + d] - A.shell_xyz[3 * dp.sh_j + d];
            CDv[d] = A.shell_xyz[3 * cd.sh_i + d] - A.shell_xyz[3 * cd.sh_j + d];
        }
        double Ep[NEP * NSCD], Em[(HASM ? NEM : 1) * NSCD];
        tpq_pair_transform<LC, LD, NEP, 1, NF, 1, NSCD>(accp, Ep, CDv, c2s + A.c2s_off[LC], c2s + A.c2s_off[LD]);
        if (HASM) tpq_pair_transform<LC, LD, NEM, 1, NF, 1, NSCD>(accm, Em, CDv, c2s + A.c2s_off[LC], c2s + A.c2s_off[LD]);
        // ---- bra per ket component: HRR (closed form) -> derivative -> cart->sph -> contraction with G
        double pw[3][L2 + 1];
#pragma unroll
        for (int d = 0; d < 3; d++) {
            pw[d][0] = 1.0;
#pragma unroll
            for (int q = 1; q <= L2; q++) pw[d][q] = pw[d][q - 1] * ABv[d];
        }
        const MI_CONST_AS double *c1 = c2s + A.c2s_off[L1], *c2 = c2s + A.c2s_off[L2];
        const double *D = A.D;
        const int ld = A.ld;
#pragma unroll
        for (int col = 0; col < NSCD; col++) {
            const int sc = col / NSD, sd = col - sc * NSD;
            // (a' b| for the plus (a' of degree LP) and minus (degree LM) shells
            double gp[NCP * NK2], gm[NCM * NK2];
#pragma unroll
            for (int pass = 0; pass < (HASM ? 2 : 1); pass++) {
                const int LX = pass == 0 ? LP : LM;
#pragma unroll
                for (int ax = LX; ax >= 0; ax--)
#pragma unroll
                    for (int ay = LX - ax; ay >= 0; ay--) {
                        const int ia = c_cidx(LX, ax, ay);
#pragma unroll
                        for (int bx = L2; bx >= 0; bx--)
#pragma unroll
                            for (int by = L2 - bx; by >= 0; by--) {
                                const int bz = L2 - bx - by, ibb = c_cidx(L2, bx, by);
                                double v = 0.0;
#pragma unroll
                                for (int ix = 0; ix <= bx; ix++)
#pragma unroll
                                    for (int iy = 0; iy <= by; iy++)
#pragma unroll
                                        for (int iz = 0; iz <= bz; iz++) {
                                            const int deg = LX + ix + iy + iz;
                                            const int e = c_eoff(LX, deg) + c_cidx(deg, ax + ix, ay + iy);
                                            const double cf = (double)(c_binom(bx, ix) * c_binom(by, iy) * c_binom(bz, iz));
                                            const double src = pass == 0 ? Ep[e * NSCD + col] : Em[(HASM ? e : 0) * NSCD + col];
                                            v = fma(cf * pw[0][bx - ix] * pw[1][by - iy] * pw[2][bz - iz], src, v);
                                        }
                                if (pass == 0) gp[ia * NK2 + ibb] = v; else gm[ia * NK2 + ibb] = v;
                            }
                    }
            }
            // density factor of this ket component for every bra component
            const int k = cd.ao_i + sc, l = cd.ao_j + sd;
            double Gd[NS1 * NS2];
#pragma unroll
            for (int sa = 0; sa < NS1; sa++)
#pragma unroll
                for (int sb = 0; sb < NS2; sb++) {
                    const int i = dp.ao_i + sa, j = dp.ao_j + sb;
                    double ex = D[(size_t)i * ld + k] * D[(size_t)j * ld + l] + D[(size_t)i * ld + l] * D[(size_t)j * ld + k];
                    if (A.Dm) ex += A.Dm[(size_t)i * ld + k] * A.Dm[(size_t)j * ld + l] + A.Dm[(size_t)i * ld + l] * A.Dm[(size_t)j * ld + k];
                    Gd[sa * NS2 + sb] = D[(size_t)i * ld + j] * D[(size_t)k * ld + l] - 0.25 * A.hyb * ex;
                    if (PAIRS) Gd[sa * NS2 + sb] += pair_term(A.pt, (size_t)i * ld + j, (size_t)k * ld + l);
                    if (XPAIRS) Gd[sa * NS2 + sb] += xpair_term(A.xt, (size_t)i * ld + k, (size_t)j * ld + l, (size_t)i * ld + l, (size_t)j * ld + k);
                }
            // Gc[a][b] = sum_{sa,sb} c1[a][sa] c2[b][sb] Gd[sa][sb]   (density back-transformed to cartesians: 3x fewer products)
            double h2[NS1 * NK2];
#pragma unroll
            for (int sa = 0; sa < NS1; sa++)
#pragma unroll
                for (int bq = 0; bq < NK2; bq++) {
                    double v = 0.0;
#pragma unroll
                    for (int sb = 0; sb < NS2; sb++) v = fma(c2[bq * NS2 + sb], Gd[sa * NS2 + sb], v);
                    h2[sa * NK2 + bq] = v;
                }
            double Gc[NK1 * NK2];
#pragma unroll
            for (int a = 0; a < NK1; a++)
#pragma unroll
                for (int bq = 0; bq < NK2; bq++) {
                    double v = 0.0;
#pragma unroll
                    for (int sa = 0; sa < NS1; sa++) v = fma(c1[a * NS1 + sa], h2[sa * NK2 + bq], v);
                    Gc[a * NK2 + bq] = v;
                }
            // derivative: d_x (a b| = (a+1_x b|_plus - a_x (a-1_x b|_minus
#pragma unroll
            for (int ax = L1; ax >= 0; ax--)
#pragma unroll
                for (int ay = L1 - ax; ay >= 0; ay--) {
                    const int az = L1 - ax - ay, ia = c_cidx(L1, ax, ay);
                    const int apow[3] = {ax, ay, az};
#pragma unroll
                    for (int xdir = 0; xdir < 3; xdir++) {
                        const int px = ax + (xdir == 0), py = ay + (xdir == 1);
                        const int ipl = c_cidx(LP, px, py);
#pragma unroll
                        for (int bq = 0; bq < NK2; bq++) {
                            double dv = gp[ipl * NK2 + bq];
                            if (HASM && apow[xdir] > 0) {
                                const int mx = ax - (xdir == 0), my = ay - (xdir == 1);
                                dv -= apow[xdir] * gm[c_cidx(LM, mx, my) * NK2 + bq];
                            }
                            force[xdir] = fma(dv, Gc[ia * NK2 + bq], force[xdir]);
                        }
                    }
                }
        }
        double wq = 4.0;
        if (dp.sh_i == dp.sh_j) wq *= 0.5;
        if (cd.sh_i == cd.sh_j) wq *= 0.5;
        if (same_pair) wq *= 0.5;
#pragma unroll
        for (int xdir = 0; xdir < 3; xdir++) force[xdir] *= wq;
    }
    // ---- forces: +f on the atom of the differentiated shell, -f on the atom of the skipped permutation.  Lanes of a wave
    // mostly share both atoms (consecutive tasks share the bra pair): reduce over the wave first when they all do.
    const int a1 = A.shell_atom[dp.sh_i], a2 = A.shell_atom[A.inv_from_second ? dp.sh_j : cd.sh_i];
    const int lane = threadIdx.x & 63;
    const bool uniform = __all(a1 == __shfl(a1, 0) && a2 == __shfl(a2, 0));
    double *gc = A.grad + (size_t)(blockIdx.x & (GRAD_COPIES - 1)) * A.natm3;
    if (uniform) {
#pragma unroll
        for (int xdir = 0; xdir < 3; xdir++) {
            double v = force[xdir];
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if (lane == 0 && v != 0.0) { atomicAdd(&gc[a1 * 3 + xdir], v); atomicAdd(&gc[a2 * 3 + xdir], -v); }
        }
    } else if (live) {
#pragma unroll
        for (int xdir = 0; xdir < 3; xdir++) { atomicAdd(&gc[a1 * 3 + xdir], force[xdir]); atomicAdd(&gc[a2 * 3 + xdir], -force[xdir]); }
    }
}

template <int L1, int L2, int LC, int LD>
static int launch_eri_tpq_grad_t(const TpqGradArgs &Q, hipStream_t st)
{
    const size_t shm = tpq_cheb_bytes((L1 + 1 + L2 + LC + LD) / 2 + 1);
    if (Q.ntask <= 0) return 1;   // nothing in this rank's share of the class (the class is still "handled")
    const dim3 grid((unsigned)((Q.ntask + TPQ_BLOCK - 1) / TPQ_BLOCK));
    return with_grad_terms(QuartetDensity{Q.D, Q.Dm, Q.ld, Q.hyb, Q.pt, Q.xt}, [&](auto terms) {
        constexpr GradTerms T = decltype(terms)::value;
        hipLaunchKernelGGL((eri_tpq_grad_kernel<L1, L2, LC, LD, T != GradTerms::PLAIN, T == GradTerms::XPAIRS>), grid, dim3(TPQ_BLOCK), shm, st, Q);
        return hipGetLastError() != hipSuccess ? fail("eri_tpq_grad_kernel launch failed") : 1;
    });
}

// returns 1 if the class (l1 = differentiated shell, l2 = partner | lc >= ld) has a thread-per-quartet kernel, 0 otherwise
// (dry = true: only answers the question)
static int launch_eri_tpq_grad(int l1, int l2, int lc, int ld, const TpqGradArgs &Q, hipStream_t st, bool dry = false)
{
    if (l1 > 3 || l2 > 3 || lc > 3 || ld > 3) return 0;
    const int key = ((l1 * 4 + l2) * 4 + lc) * 4 + ld;
#define TPQG_CASE(a, b, c_, d) case (((a) * 4 + (b)) * 4 + (c_)) * 4 + (d): return dry ? 1 : launch_eri_tpq_grad_t<a, b, c_, d>(Q, st)
    switch (key) {
        // other pair (ss)
        TPQG_CASE(0, 0, 0, 0); TPQG_CASE(1, 0, 0, 0); TPQG_CASE(0, 1, 0, 0); TPQG_CASE(1, 1, 0, 0); TPQG_CASE(2, 0, 0, 0);
        TPQG_CASE(2, 1, 0, 0); TPQG_CASE(1, 2, 0, 0); TPQG_CASE(3, 0, 0, 0); TPQG_CASE(2, 2, 0, 0);
        TPQG_CASE(3, 1, 0, 0);   // (sd|ss), (sf|ss), (pf|ss): the compiler leaves their index arrays in scratch -> wave-per-quartet path
        // other pair (ps)
        TPQG_CASE(0, 0, 1, 0); TPQG_CASE(1, 0, 1, 0); TPQG_CASE(0, 1, 1, 0); TPQG_CASE(1, 1, 1, 0); TPQG_CASE(2, 0, 1, 0); TPQG_CASE(0, 2, 1, 0);
        TPQG_CASE(3, 0, 1, 0);
        // other pair (pp), (ds), (fs), (dp): (NEP + NEM) * NF accumulators <= ~64
        TPQG_CASE(0, 0, 1, 1); TPQG_CASE(1, 0, 1, 1);
        TPQG_CASE(0, 0, 2, 0); TPQG_CASE(1, 0, 2, 0); TPQG_CASE(0, 1, 2, 0);
        TPQG_CASE(0, 0, 3, 0);
        TPQG_CASE(0, 0, 2, 1);
        // round 3: candidates with up to ~150 accumulators (one wave per SIMD); kept only where the compiler needs no scratch
        TPQG_CASE(0, 1, 1, 1); TPQG_CASE(1, 0, 3, 0); TPQG_CASE(0, 1, 3, 0); TPQG_CASE(1, 1, 2, 0);
        TPQG_CASE(1, 0, 2, 1); TPQG_CASE(0, 1, 2, 1); TPQG_CASE(2, 0, 2, 0); TPQG_CASE(1, 2, 1, 0); TPQG_CASE(0, 2, 2, 0);
        TPQG_CASE(2, 0, 1, 1); TPQG_CASE(0, 0, 3, 1); TPQG_CASE(0, 0, 2, 2);
        TPQG_CASE(2, 1, 1, 0);
    default: return 0;
    }
#undef TPQG_CASE
}

static bool tpq_grad_has_class(int l1, int l2, int lc, int ld)
{
    TpqGradArgs none{};
    return launch_eri_tpq_grad(l1, l2, lc, ld, none, nullptr, true) == 1;
}

// max |D| over the AO block of every shell pair (density-weighted screening of the derivative quartets)
__global__ void shell_dmax_kernel(const double *D, const double *Dm, int ld, const int *sh_ao, const int *sh_n, int nbas, double *out)
{
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nbas * nbas) return;
    int a = idx / nbas, b = idx - a * nbas;
    double m = 0.0;
    for (int i = 0; i < sh_n[a]; i++)
        for (int j = 0; j < sh_n[b]; j++) {
            size_t o = (size_t)(sh_ao[a] + i) * ld + sh_ao[b] + j;
            // open shell: |D| + |M| bounds both spin densities (the exchange bound then covers D x D + M x M)
            m = fmax(m, fabs(D[o]) + (Dm ? fabs(Dm[o]) : 0.0));
        }
    out[idx] = m;
}

// pair mode: P[(r * ld + c) * K + k] = w[k] * Q[src[k]][iperm[r]][iperm[c]] (w = sqrt|s|, zero in the padding)
__global__ void pad_pairs_kernel(const double *Q, const int *src, const double *w, int K, double *P, int nao, int ld, const int *__restrict__ iperm)
{
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)ld * ld * K) return;
    const int k = (int)(idx % K);
    const int64_t rc = idx / K;
    const int r = (int)(rc / ld), c = (int)(rc - (int64_t)r * ld);
    P[idx] = (r < nao && c < nao) ? w[k] * Q[((size_t)src[k] * nao + iperm[r]) * nao + iperm[c]] : 0.0;
}
// qmax_ab = sqrt(sum_k max_{ab} P_k^2) per shell pair (see quartet_density_bound)
__global__ void shell_qmax_kernel(const double *P, int K, int ld, const int *sh_ao, const int *sh_n, int nbas, double *out)
{
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nbas * nbas) return;
    int a = idx / nbas, b = idx - a * nbas;
    double sum = 0.0;
    for (int k = 0; k < K; k++) {
        double m = 0.0;
        for (int i = 0; i < sh_n[a]; i++)
            for (int j = 0; j < sh_n[b]; j++) m = fmax(m, fabs(P[((size_t)(sh_ao[a] + i) * ld + sh_ao[b] + j) * K + k]));
        sum += m * m;
    }
    out[idx] = sqrt(sum);
}

__global__ void grad_reduce_copies_kernel(const double *copies, int natm3, double *grad)
{
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= natm3) return;
    double s = 0.0;
    for (int c = 0; c < GRAD_COPIES; c++) s += copies[(size_t)c * natm3 + idx];
    grad[idx] += s;
}

// eri_grad_contract for one batch of `nb` quartets whose [e0|f0] blocks are in X.work_p / X.work_m, shared by the four-centre
// and the density-fitted (df) gradient: four quartets per wave for the small classes (four-centre only), else one wave per
// quartet, on the matrix cores where one of the three products is large enough.
static int launch_grad_contract(bool df, const GradXfArgs &X, bool has_m, int nb, size_t shm, hipStream_t st)
{
    const int big = std::max({X.ns1 * X.ns2 * X.nscd, X.ns1 * X.ns2 * X.nf, X.ns1 * X.ns2 * X.ne_p});
    const bool mfma = mfma_worthwhile(X.ns1 * X.ns2, X.nf, X.nscd) || mfma_worthwhile(X.ns1 * X.ns2, X.ne_p, X.nf) ||
                      (has_m && mfma_worthwhile(X.ns1 * X.ns2, X.ne_m, X.nf));
    auto launch = [&](auto kernel, int grid, size_t bytes) {
        if (bytes > 64 * 1024) HIPCHK(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), bytes, st, X);
        HIPCHK(hipGetLastError());
        return 0;
    };
    if (df) return mfma ? launch(eri_grad_contract<64, true, true>, nb, shm) : launch(eri_grad_contract<64, false, true>, nb, shm);
    return with_grad_terms(X.dens, [&](auto terms) {   // the same three geometries in every mode
        constexpr GradTerms T = decltype(terms)::value;
        // small classes: four quartets per wave (16 lanes each)
        if (big <= 48 && shm * 4 <= 64 * 1024) return launch(eri_grad_contract<16, false, false, T>, (nb + 3) / 4, shm * 4);
        // (two or four waves sharing one quartet's LDS blocks -- eri_grad_contract<128|256, true> -- were measured at
        // -2 % / +8 %, the six density sub-blocks of G staged in LDS first at +2 %: the kernel is parked 70 % of its
        // wave cycles, but neither on a shortage of lanes nor on the G gather)
        return mfma ? launch(eri_grad_contract<64, true, false, T>, nb, shm) : launch(eri_grad_contract<64, false, false, T>, nb, shm);
    });
}

// ---- mi_grad_eri_sharded: the per-call buffers (GradState), one (bra class, ket class) pair (GradClassPair), one of its role
// permutations (GradPerm), and the three routes a permutation is offered to in turn -- thread per quartet, row kernel,
// Rys -> hand-over -> contraction pipeline; each returns 1 (handled), 0 (not its class) or -1 (error).
struct GradState {
    mi_ctx *c;
    hipStream_t st;
    int rank, nranks;
    int natm3;
    size_t work_doubles = 0;                 // per hand-over buffer (plus / minus)
    DevBuf<double> d_Mpad;                   // spin density Da - Db, padded like D (open shell only)
    DevBuf<int> d_shell_atom, d_sh_ao, d_sh_n;
    DevBuf<double> d_dmax;                   // max |D| per shell pair (null: no density-weighted screening)
    DevBuf<double> d_gcopies;
    DevBuf<double> d_P, d_qmax;              // pair mode: sqrt|s_k| Q^k, k fastest (PairTerm), and its per-shell-pair bound
    DevBuf<double> d_X, d_xmax;              // exchange-pair mode: sqrt|t_m| R^m, m fastest, and its per-shell-pair bound
    QuartetDensity dens{};                   // what every kernel of this call contracts with
    QuartetScreen scr{};                     // prototype: q_bra, q_ket and dmax vary per route (screen)
    // the screen of the launches over (differentiated pair class Dc | other pair class Oc); dmax null: the task list is already screened
    QuartetScreen screen(const PairClass &Dc, const PairClass &Oc, const double *dmax) const
    {
        QuartetScreen s = scr;
        s.q_bra = Dc.d_q; s.q_ket = Oc.d_q; s.dmax = dmax;
        return s;
    }
    Scratch scr_wp, scr_wm, scr_gtasks, scr_live;
    DevBuf<uint32_t> d_comp_p, d_comp_m;
    DevBuf<int64_t> d_prefix;
    DevBuf<int> d_live_counts;
    DevBuf<int64_t> d_live_off;
    int64_t batch_counter = 0;               // pipeline batches are dealt round-robin to the ranks
};
struct GradClassPair {
    PairClass *B, *Kc;
    bool same;
    int64_t ntask;
    bool live_ok;                // the class pair may build the list of live quartets (grad_ensure_live)
    int64_t nlive = -1;          // its length once built
    const TaskIdx *tasks_dev = nullptr;   // (bra, ket) table of all tasks, where one was written
};
struct GradPerm {
    int perm, orient;
    bool swap;
    PairClass *Dc, *Oc;          // class of the differentiated pair / of the other pair (plain ket)
    int l1, l2, lc, ld;
    bool has_m;                  // an (l1 - 1) variant exists
    // what the wave-per-quartet launches (row kernel, pipeline) walk: the live list when there is one
    int64_t ntask_w;
    const TaskIdx *tasks_w;
    const double *dmax_w;        // null: the live list is already screened
    EriArgs Ep, Em;
};

// wave-per-quartet launches of a class pair walk the list of LIVE quartets (density-weighted screening done once, see
// live_fill_kernel); built on first need -- classes wholly on the thread-per-quartet path never ask for it
static int grad_ensure_live(GradState &G, GradClassPair &CP)
{
    mi_ctx *c = G.c;
    hipStream_t st = G.st;
    const PairClass &B = *CP.B, &Kc = *CP.Kc;
    const int64_t ntask = CP.ntask;
    // (lists beyond 2^28 quartets -- 2 GB -- are not built: those launches screen per wave as before)
    if (CP.nlive >= 0 || !CP.live_ok) return 0;
    const int nblk = (int)((ntask + 255) / 256);
    if ((size_t)nblk + 1 > G.d_live_counts.cap) {
        const size_t live_cap = (size_t)nblk + 1 + (size_t)nblk / 4;
        HIPCHK(G.d_live_counts.alloc(live_cap));
        HIPCHK(G.d_live_off.alloc(live_cap));
    }
    if (G.scr_live.ensure(c->device, SCR_GRAD_LIVE, sizeof(TaskIdx) * (size_t)ntask)) return -1;
    TaskIdx *d_live_tasks = (TaskIdx *)G.scr_live.p;
    LiveArgs L{B.d_recs, Kc.d_recs, G.d_prefix, (int)B.recs.size(), ntask, G.screen(B, Kc, G.d_dmax)};
    hipLaunchKernelGGL(live_count_kernel, dim3(nblk), dim3(256), 0, st, L, G.d_live_counts.get());
    hipLaunchKernelGGL(live_scan_kernel, dim3(1), dim3(1024), 0, st, G.d_live_counts.get(), nblk, G.d_live_off.get());
    hipLaunchKernelGGL(live_fill_kernel, dim3(nblk), dim3(256), 0, st, L, G.d_live_off.get(), d_live_tasks);
    HIPCHK(hipGetLastError());
    int64_t n = 0;
    HIPCHK(hipMemcpyAsync(&n, G.d_live_off + nblk, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    CP.nlive = n;
    if (getenv("MI355_DEBUG"))
        fprintf(stderr, "[mi355] grad class pair (%d%d|%d%d): %ld of %ld quartets live\n", B.la, B.lb, Kc.la, Kc.lb, (long)CP.nlive, (long)ntask);
    return 0;
}

// low classes, shallow contraction: thread per (quartet, permutation)
static int grad_route_tpq(GradState &G, GradClassPair &CP, const GradPerm &M)
{
    mi_ctx *c = G.c;
    hipStream_t st = G.st;
    const PairClass &B = *CP.B, &Kc = *CP.Kc, &Dc = *M.Dc, &Oc = *M.Oc;
    const int64_t ntask = CP.ntask;
    if (!(c->opt_eri_tpq && B.mean_np * Kc.mean_np <= c->opt_tpq_maxprim && ntask >= c->opt_tpq_min_tasks)) return 0;
    TpqGradArgs Q{};
    Q.dplus = Dc.d_g_recs[M.orient][0]; Q.dminus = M.l1 >= 1 ? Dc.d_g_recs[M.orient][1] : nullptr; Q.ket = Oc.d_recs;
    Q.prim = c->d_prim; Q.prefix = G.d_prefix; Q.nbra = (int)B.recs.size();
    // this rank's contiguous share of the task list (the compacted live list when the class has a kernel)
    const bool has_tpq = tpq_grad_has_class(M.l1, M.l2, M.lc, M.ld);
    if (has_tpq && grad_ensure_live(G, CP)) return -1;
    const bool live_q = has_tpq && CP.nlive >= 0;
    const int64_t nt_q = live_q ? CP.nlive : ntask;
    const int64_t lo_t = nt_q * G.rank / G.nranks, hi_t = nt_q * (G.rank + 1) / G.nranks;
    Q.t0 = lo_t; Q.ntask = hi_t - lo_t;
    Q.tasks = live_q ? (const TaskIdx *)G.scr_live.p : nullptr;
    Q.swap = M.swap ? 1 : 0; Q.same_class = CP.same;
    Q.c2s = c->d_c2s;
    for (int q = 0; q <= LMAX + 1; q++) Q.c2s_off[q] = c->c2s_off[q];
    Q.rys = c->rys; Q.shell_xyz = c->d_shell_xyz; Q.D = G.dens.D; Q.Dm = G.dens.Dm; Q.ld = G.dens.ld; Q.hyb = G.dens.hyb;
    Q.shell_atom = G.d_shell_atom; Q.grad = G.d_gcopies; Q.natm3 = G.natm3; Q.inv_from_second = M.swap ? 0 : 1;
    Q.q_bra = Dc.d_q; Q.q_ket = Oc.d_q; Q.dmax = live_q ? nullptr : G.d_dmax.get(); Q.nbas_d = c->nbas; Q.dtol = c->opt_grad_dtol;
    Q.qmax = G.d_qmax; Q.pt = G.dens.pt; Q.xmax = G.d_xmax; Q.xt = G.dens.xt;
    const bool dbg1 = getenv("MI355_DEBUG") != nullptr;
    auto tq0 = std::chrono::steady_clock::now();
    if (dbg1) hipStreamSynchronize(st);
    const int used = launch_eri_tpq_grad(M.l1, M.l2, M.lc, M.ld, Q, st);
    if (used > 0 && dbg1) {
        hipStreamSynchronize(st);
        fprintf(stderr, "[mi355] grad class (%d%d|%d%d) perm %d: %ld quartets, %.3f s (thread per quartet)\n", M.l1, M.l2, M.lc, M.ld, M.perm,
                (long)ntask, std::chrono::duration<double>(std::chrono::steady_clock::now() - tq0).count());
    }
    return used;
}

// row kernel: no hand-over, one launch (see eri_grad_rows_kernel)
static int grad_route_rows(GradState &G, const GradClassPair &CP, const GradPerm &M)
{
    mi_ctx *c = G.c;
    hipStream_t st = G.st;
    const PairClass &B = *CP.B, &Dc = *M.Dc, &Oc = *M.Oc;
    const int l1 = M.l1, l2 = M.l2, lc = M.lc, ldd = M.ld;
    if (!c->opt_grad_rows) return 0;
    const int ne_p = ne_of(l1 + 1, l2), ne_m = M.has_m ? ne_of(l1 - 1, l2) : 0, ne_all = ne_p + ne_m;
    GradRowsArgs R{};
    if (!(ne_all >= c->opt_grad_rows_min && launch_grad_rows(lc, ldd, ne_all, R, 0, st, true) == 1)) return 0;
    R.dplus = Dc.d_g_recs[M.orient][0]; R.dminus = M.has_m ? Dc.d_g_recs[M.orient][1] : nullptr; R.ket = Oc.d_recs;
    R.prim = c->d_prim; R.Mbuf = c->d_M; R.tasks = M.tasks_w; R.prefix = G.d_prefix; R.nbra = (int)B.recs.size();
    const int64_t lo_t = M.ntask_w * G.rank / G.nranks, hi_t = M.ntask_w * (G.rank + 1) / G.nranks;
    R.t0 = lo_t; R.ntask = hi_t - lo_t;
    R.swap = M.swap ? 1 : 0; R.same_class = CP.same;
    const RowsGeom gm = rows_geometry(ne_all);
    R.nmax = M.Ep.nmax; R.nroots = M.Ep.nroots; R.tsz = M.Ep.tsz; R.PB = std::max(1, gm.gsz / (3 * M.Ep.nroots));
    R.ne_p = ne_p; R.ne_m = ne_m; R.nsab = (2 * l1 + 1) * (2 * l2 + 1); R.ns2 = 2 * l2 + 1;
    R.comp_p = G.d_comp_p; R.comp_m = G.d_comp_m; R.rys = c->rys;
    R.shell_atom = G.d_shell_atom; R.grad = G.d_gcopies; R.natm3 = G.natm3;
    R.inv_from_second = M.swap ? 0 : 1;
    R.dens = G.dens; R.scr = G.screen(Dc, Oc, M.dmax_w);
    const int nscd_ = Oc.nsab, nf_ = Oc.ne;
    const size_t shm_q = sizeof(double) * (RysLds{R.PB, R.nroots, R.tsz}.doubles() + grad_rows_lds_extra(R.PB, nscd_, nf_, R.nsab));
    if (!(R.ntask < ((int64_t)1 << 31))) return 0;
    const bool dbgr = getenv("MI355_DEBUG") != nullptr;
    auto tr0 = std::chrono::steady_clock::now();
    if (dbgr) hipStreamSynchronize(st);
    const int used = R.ntask > 0 ? launch_grad_rows(lc, ldd, ne_all, R, shm_q, st) : 1;
    if (used > 0 && dbgr) {
        hipStreamSynchronize(st);
        fprintf(stderr, "[mi355] grad class (%d%d|%d%d) perm %d: %ld quartets, %.4f s (row kernel, %d rows x %d lanes)\n", l1, l2, lc,
                ldd, M.perm, (long)M.ntask_w, std::chrono::duration<double>(std::chrono::steady_clock::now() - tr0).count(), gm.rows, gm.gsz);
    }
    return used;
}

// everything else: two Rys launches (l+1, l-1) -> hand-over buffers -> eri_grad_contract, batch by batch
static int grad_route_pipeline(GradState &G, const GradClassPair &CP, GradPerm &M)
{
    mi_ctx *c = G.c;
    hipStream_t st = G.st;
    const PairClass &B = *CP.B, &Kc = *CP.Kc, &Dc = *M.Dc, &Oc = *M.Oc;
    const int l1 = M.l1, l2 = M.l2, lc = M.lc, ldd = M.ld, rank = G.rank, nranks = G.nranks;
    const bool has_m = M.has_m;
    EriArgs &Ep = M.Ep, &Em = M.Em;
    Ep.tasks = Em.tasks = M.tasks_w;
    Ep.prim_lds = Em.prim_lds = (c->opt_prim_lds && B.max_np + Kc.max_np <= 160) ? B.max_np + Kc.max_np : 0;
    Ep.h_shared_np = B.mean_np; Ep.h_vary_mean = Kc.mean_np; Ep.h_vary_max4 = Kc.max4_np;
    Em.h_shared_np = B.mean_np; Em.h_vary_mean = Kc.mean_np; Em.h_vary_max4 = Kc.max4_np;
    GradXfArgs X{};
    X.dens = G.dens; X.scr = Ep.scr = G.screen(Dc, Oc, M.dmax_w);
    if (has_m) Em.scr = Ep.scr;
    X.dplus = Dc.d_g_recs[M.orient][0]; X.dminus = has_m ? Dc.d_g_recs[M.orient][1] : nullptr; X.ket = Oc.d_recs;
    X.Mbuf = c->d_M; X.prefix = G.d_prefix; X.nbra = Ep.nbra; X.swap = Ep.swap; X.same_class = CP.same;
    X.ne_p = ne_of(l1 + 1, l2); X.ne_m = has_m ? ne_of(l1 - 1, l2) : 0; X.nf = Oc.ne;
    X.ns1 = 2 * l1 + 1; X.ns2 = 2 * l2 + 1; X.nscd = Oc.nsab; X.nsd = 2 * Oc.lb + 1;
    X.work_p = (double *)G.scr_wp.p; X.work_m = (double *)G.scr_wm.p; X.ncomp_p = Ep.ncomp; X.ncomp_m = has_m ? Em.ncomp : 0;
    X.shell_atom = G.d_shell_atom; X.grad = G.d_gcopies; X.natm3 = G.natm3;
    X.inv_from_second = M.swap ? 0 : 1;
    X.tasks = M.tasks_w;
    size_t shm = sizeof(double) * ((size_t)X.ne_p * X.nf + (size_t)X.ne_m * X.nf + (size_t)X.ns1 * X.ns2 * (X.nf + X.nscd));
    if (shm > 160 * 1024) return fail("gradient contraction needs %zu bytes of LDS", shm);
    const bool dbg = getenv("MI355_DEBUG") != nullptr;
    auto tc0 = std::chrono::steady_clock::now();
    if (dbg) hipStreamSynchronize(st);
    int64_t per = std::min<int64_t>((int64_t)(G.work_doubles / Ep.ncomp), (int64_t)1 << 23);
    if (nranks > 1) per = std::min<int64_t>(per, std::max<int64_t>(1024, M.ntask_w / (8 * nranks)));
    for (int64_t t0 = 0; t0 < M.ntask_w; t0 += per) {
        if ((int)((G.batch_counter++) % nranks) != rank) continue; // batches dealt round-robin to ranks
        int nb = (int)std::min<int64_t>(per, M.ntask_w - t0);
        Ep.t0 = t0; Ep.ntask = nb;
        if (launch_eri(c, Ep, nb, st)) return -1;
        if (has_m) { Em.t0 = t0; Em.ntask = nb; if (launch_eri(c, Em, nb, st)) return -1; }
        X.t0 = t0; X.nbatch = nb;
        if (launch_grad_contract(false, X, has_m, nb, shm, st)) return -1;
    }
    if (dbg) {
        hipStreamSynchronize(st);
        fprintf(stderr, "[mi355] grad class (%d%d|%d%d) perm %d: %ld quartets, %.3f s\n", l1, l2, lc, ldd, M.perm, (long)CP.ntask,
                std::chrono::duration<double>(std::chrono::steady_clock::now() - tc0).count());
    }
    return 1;
}

// one role permutation of a class pair: derivative on the first shell of (ji|kl), (kl|ij) or (lk|ij)
static int grad_permutation(GradState &G, GradClassPair &CP, int perm)
{
    mi_ctx *c = G.c;
    hipStream_t st = G.st;
    PairClass &B = *CP.B, &Kc = *CP.Kc;
    GradPerm M{};
    M.perm = perm;
    M.swap = perm >= 2;
    M.orient = perm & 1;
    M.Dc = M.swap ? &Kc : &B;
    M.Oc = M.swap ? &B : &Kc;
    const PairClass &Dc = *M.Dc, &Oc = *M.Oc;
    M.l1 = M.orient == 0 ? Dc.la : Dc.lb; M.l2 = M.orient == 0 ? Dc.lb : Dc.la;
    M.lc = Oc.la; M.ld = Oc.lb;
    M.has_m = M.l1 >= 1;
    int used = grad_route_tpq(G, CP, M);
    if (used) return used < 0 ? -1 : 0;
    if (grad_ensure_live(G, CP)) return -1;
    const bool use_live = CP.nlive >= 0;
    if (use_live && CP.nlive == 0) return 0;
    M.ntask_w = use_live ? CP.nlive : CP.ntask;            // tasks the wave-per-quartet launches walk
    M.tasks_w = use_live ? (const TaskIdx *)G.scr_live.p : CP.tasks_dev;
    M.dmax_w = use_live ? nullptr : G.d_dmax.get();          // the live list is already screened
    if (upload_comp_table(M.l1 + 1, M.l2, M.lc, M.ld, G.d_comp_p, st)) return -1;
    if (M.has_m && upload_comp_table(M.l1 - 1, M.l2, M.lc, M.ld, G.d_comp_m, st)) return -1;
    M.Ep = eri_class_args(c, M.l1 + 1, M.l2, M.lc, M.ld, Dc.d_g_recs[M.orient][0], Oc.d_recs, c->d_prim, G.d_prefix, (int)B.recs.size(),
                          G.d_comp_p, (double *)G.scr_wp.p);
    M.Ep.swap = M.swap ? 1 : 0;
    if (M.has_m) {
        M.Em = eri_class_args(c, M.l1 - 1, M.l2, M.lc, M.ld, Dc.d_g_recs[M.orient][1], Oc.d_recs, c->d_prim, G.d_prefix, M.Ep.nbra,
                              G.d_comp_m, (double *)G.scr_wm.p);
        M.Em.swap = M.Ep.swap;
    }
    used = grad_route_rows(G, CP, M);
    if (!used) used = grad_route_pipeline(G, CP, M);
    return used < 0 ? -1 : 0;
}

static int grad_class_pair(GradState &G, PairClass &B, PairClass &Kc, bool same)
{
    mi_ctx *c = G.c;
    hipStream_t st = G.st;
    std::vector<int64_t> prefix;
    GradClassPair CP{};
    CP.B = &B; CP.Kc = &Kc; CP.same = same; CP.nlive = -1;
    const int64_t ntask = CP.ntask = class_prefix(B, Kc, same, c->tol, prefix);
    if (ntask == 0) return 0;
    if (prefix_to_device(prefix, G.d_prefix, st)) return -1;
    CP.live_ok = G.d_dmax && c->opt_grad_live && ntask >= 4096 && ntask <= ((int64_t)1 << 28);   // see grad_ensure_live
    if (c->opt_task_table && ntask >= 65536 && ntask <= ((int64_t)1 << 28) && !CP.live_ok) {   // up to 3 permutations x 3 launches walk this task list
        if (G.scr_gtasks.ensure(c->device, SCR_GRAD_TASKS, sizeof(TaskIdx) * (size_t)ntask)) return -1;
        hipLaunchKernelGGL(fill_tasks_kernel, dim3((unsigned)((ntask + 255) / 256)), dim3(256), 0, st, G.d_prefix.get(), (int)B.recs.size(), ntask,
                           (TaskIdx *)G.scr_gtasks.p);
        CP.tasks_dev = (const TaskIdx *)G.scr_gtasks.p;
    }
    HIPCHK(hipStreamSynchronize(st));
    // perm 0 (derivative on P.sh_i, the costliest: highest l) is skipped: sum of the four forces = 0
    for (int perm = 1; perm < 4; perm++)
        if (grad_permutation(G, CP, perm)) return -1;
    return 0;
}

// Pair / exchange-pair mode: the matrices of `d_src` whose coefficient is not zero, the positive ones first, scaled by
// sqrt|coef| and laid out term fastest in `store` (PairTerm).  No such matrix: `out` stays empty.
static int stage_pair_term(mi_ctx *c, hipStream_t st, const double *d_src, const double *coef, int K, DevBuf<double> &store, PairTerm &out,
                           const char *oom_fmt)
{
    std::vector<int> src;
    std::vector<double> w;
    int npos = 0;
    for (int sign = 0; sign < 2; sign++)
        for (int k = 0; k < K; k++)
            if (sign == 0 ? coef[k] > 0.0 : coef[k] < 0.0) { src.push_back(k); w.push_back(sqrt(fabs(coef[k]))); npos += sign == 0; }
    const int Ke = (int)src.size();
    if (Ke == 0) return 0;
    const size_t pp = (size_t)c->ldp * c->ldp;
    DevBuf<int> d_idx;   // (these two are freed on return with pad_pairs_kernel possibly still queued: safe because dev_free
    DevBuf<double> d_w;  // synchronises the device before it parks a block -- one synchronisation per staged term list)
    if (d_idx.upload(src) || d_w.upload(w)) return -1;
    if (store.alloc(pp * Ke) != hipSuccess) return fail(oom_fmt, Ke);
    hipLaunchKernelGGL(pad_pairs_kernel, dim3((unsigned)((pp * Ke + 255) / 256)), dim3(256), 0, st, d_src, d_idx.get(), d_w.get(), Ke, store.get(),
                       c->nao, c->ldp, c->d_iperm);
    HIPCHK(hipGetLastError());
    out = PairTerm{store.get(), Ke, npos};
    return 0;
}
// the per-shell-pair bound of a staged term (see quartet_density_bound); no term: `out` stays null
static int pair_term_bound(GradState &G, const PairTerm &T, DevBuf<double> &out)
{
    if (!T.P) return 0;
    const int nb2 = G.c->nbas * G.c->nbas;
    HIPCHK(out.alloc((size_t)nb2));
    hipLaunchKernelGGL(shell_qmax_kernel, dim3((nb2 + 255) / 256), dim3(256), 0, G.st, T.P, T.K, G.c->ldp, G.d_sh_ao.get(), G.d_sh_n.get(),
                       G.c->nbas, out.get());
    return 0;
}
// what both public entries ask of a list of `K` signed terms (`names`: how the messages spell the count and the coefficients;
// sym: the symmetry flags of exchange-pair terms, checked term by term with the coefficients)
static int check_terms(const char *who, const char *const names[2], const void *ptr, const double *coef, int K, int Kmax, const int *sym = nullptr)
{
    if (K < 0 || K > Kmax) return fail("%s: %s = %d outside 0 .. %d", who, names[0], K, Kmax);
    if (K > 0 && (!ptr || !coef)) return fail("%s: null argument", who);
    for (int k = 0; k < K; k++) {
        if (!std::isfinite(coef[k])) return fail("%s: %s[%d] is not finite", who, names[1], k);
        if (sym && sym[k] != 1 && sym[k] != -1) return fail("%s: sym[%d] = %d is neither +1 (symmetric) nor -1 (antisymmetric)", who, k, sym[k]);
    }
    return 0;
}
static const char *const PAIR_NAMES[2] = {"K", "s"}, *const XPAIR_NAMES[2] = {"Kx", "t"};

// (rank, nranks): which share of the derivative-quartet batches this call evaluates.  It is an ARGUMENT, not the split of
// the last mi_eri_prepare: in direct mode the tile store is prepared group by group (rank*ng + v of nranks*ng) while the
// gradient is still shared between the nranks processes only.
// d_Q / s / K: the pair term of mi_grad_eri_pairs (K = 0: none, the plain Hartree-Fock form)
// d_R / t / Kx: the exchange-pair term of mi_grad_eri_xpairs (Kx = 0: none)
static int grad_eri_run(mi_ctx *c, const double *d_D, const double *d_Dspin, double hyb, const double *d_Q, const double *s, int K,
                        double *d_grad, int rank, int nranks, void *stream, const double *d_R = nullptr, const double *t = nullptr, int Kx = 0)
{
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail("mi_grad_eri: bad rank/nranks");
    if (!c || !d_D || !d_grad) return fail("mi_grad_eri: null argument");
    if (c->opt_omega != 0.0 || c->eri_omega != 0.0) return fail("mi_grad_eri: no derivative integrals for a long-range (omega != 0) context");
    if (!c->eri_ready) return fail("mi_grad_eri: call mi_eri_prepare first");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    auto tg0 = std::chrono::steady_clock::now();
    if (prepare_grad_records(c)) return -1;
    auto tg1 = std::chrono::steady_clock::now();
    GradState G;
    G.c = c; G.st = st; G.rank = rank; G.nranks = nranks; G.natm3 = c->natm * 3;
    size_t pp = (size_t)c->ldp * c->ldp;
    double *const none = nullptr;   // no accumulators to clear
    hipLaunchKernelGGL(pad_density_clear_kernel, dim3((unsigned)((pp + 255) / 256)), dim3(256), 0, st, d_D, c->d_Dpad, none, none, c->nao, c->ldp, c->d_iperm);
    if (d_Dspin) {
        HIPCHK(G.d_Mpad.alloc(pp));
        hipLaunchKernelGGL(pad_density_clear_kernel, dim3((unsigned)((pp + 255) / 256)), dim3(256), 0, st, d_Dspin, G.d_Mpad.get(), none, none, c->nao, c->ldp, c->d_iperm);
    }
    std::vector<int> shell_atom(c->nbas);
    for (int i = 0; i < c->nbas; i++) shell_atom[i] = c->shells[i].atom;
    if (G.d_shell_atom.upload(shell_atom)) return -1;
    G.dens = QuartetDensity{c->d_Dpad, G.d_Mpad, c->ldp, hyb, {nullptr, 0, 0}, {nullptr, 0, 0}};
    if (stage_pair_term(c, st, d_Q, s, K, G.d_P, G.dens.pt, "mi_grad_eri_pairs: no memory for %d pair matrices") ||
        stage_pair_term(c, st, d_R, t, Kx, G.d_X, G.dens.xt, "mi_grad_eri_xpairs: no memory for %d exchange-pair matrices"))
        return -1;
    // density-weighted screening: q_ab q_cd max|G| < grad_dtol skips the quartet (0 disables)
    if (c->opt_grad_dtol > 0.0) {
        std::vector<int> sh_ao(c->nbas), sh_n(c->nbas);
        for (int i = 0; i < c->nbas; i++) { sh_ao[i] = c->shells[i].ao; sh_n[i] = 2 * c->shells[i].l + 1; }
        if (G.d_sh_ao.upload(sh_ao) || G.d_sh_n.upload(sh_n)) return -1;
        // (|R^m_ab| = |R^m_ba|, symmetric or antisymmetric: one bound serves both orientations of a quartet)
        if (pair_term_bound(G, G.dens.pt, G.d_qmax) || pair_term_bound(G, G.dens.xt, G.d_xmax)) return -1;
        HIPCHK(G.d_dmax.alloc((size_t)c->nbas * c->nbas));
        hipLaunchKernelGGL(shell_dmax_kernel, dim3((c->nbas * c->nbas + 255) / 256), dim3(256), 0, st, c->d_Dpad, G.d_Mpad.get(), c->ldp,
                           G.d_sh_ao.get(), G.d_sh_n.get(), c->nbas, G.d_dmax.get());
        HIPCHK(hipGetLastError());
    }
    G.scr = QuartetScreen{nullptr, nullptr, nullptr, G.d_qmax, G.d_xmax, c->nbas, c->opt_grad_dtol, hyb};
    const int natm3 = G.natm3;
    HIPCHK(G.d_gcopies.alloc((size_t)GRAD_COPIES * natm3));
    HIPCHK(hipMemsetAsync(G.d_gcopies, 0, sizeof(double) * (size_t)GRAD_COPIES * natm3, st));
    G.work_doubles = (size_t)8 << 17; // per buffer (plus / minus): what the molecule can need, at most `grad_work_mb`
    {
        const size_t cap = (size_t)std::max(8, c->opt_grad_work_mb) << 17;
        for (int bc = 0; bc < NPC; bc++)
            for (int kc = 0; kc <= bc; kc++) {
                const PairClass &B = c->pc[bc], &Kc = c->pc[kc];
                const int ne_up = std::max(ne_of(B.la + 1, B.lb), ne_of(Kc.la + 1, Kc.lb));
                const double need = (double)B.recs.size() * (double)Kc.recs.size() * (double)ne_up * (double)std::max(B.ne, Kc.ne);
                G.work_doubles = (size_t)std::min<double>((double)cap, std::max<double>((double)G.work_doubles, need));
            }
    }
    if (G.scr_wp.ensure(c->device, SCR_GRAD_WP, sizeof(double) * G.work_doubles) || G.scr_wm.ensure(c->device, SCR_GRAD_WM, sizeof(double) * G.work_doubles)) return -1;
    HIPCHK(G.d_comp_p.alloc(COMP_CAP));
    HIPCHK(G.d_comp_m.alloc(COMP_CAP));
    for (int bc = 0; bc < NPC; bc++)
        for (int kc = 0; kc <= bc; kc++) {
            PairClass &B = c->pc[bc], &Kc = c->pc[kc];
            if (B.recs.empty() || Kc.recs.empty()) continue;
            if (grad_class_pair(G, B, Kc, bc == kc)) return -1;
        }
    hipLaunchKernelGGL(grad_reduce_copies_kernel, dim3((natm3 + 63) / 64), dim3(64), 0, st, G.d_gcopies.get(), natm3, d_grad);
    HIPCHK(hipStreamSynchronize(st));
    if (getenv("MI355_DEBUG"))
        fprintf(stderr, "[mi355] grad_eri: variant records %.3f s, derivative quartets %.3f s\n",
                std::chrono::duration<double>(tg1 - tg0).count(),
                std::chrono::duration<double>(std::chrono::steady_clock::now() - tg1).count());
    return 0;   // (the buffers of G go back to the pool, its Scratch handles to the per-device cache)
}

extern "C" int mi_grad_eri_sharded(mi_ctx *c, const double *d_D, const double *d_Dspin, double hyb, double *d_grad, int rank, int nranks,
                                   void *stream)
{
    return grad_eri_run(c, d_D, d_Dspin, hyb, nullptr, nullptr, 0, d_grad, rank, nranks, stream);
}

// Gradient of  1/2 D.J[D] - hyb/4 (D.K[D] + M.K[M]) + 1/2 sum_k s_k (Q^k|Q^k)  in one pass over the derivative quartets: the
// two-particle density of every quartet is the Hartree-Fock form plus sum_k s_k Q^k_ab Q^k_cd (symmetric Q^k; the active-space
// cumulant of a CAS wavefunction, casscf_grad.py).  K = 0 is mi_grad_eri_sharded.
extern "C" int mi_grad_eri_pairs(mi_ctx *c, const double *d_D, const double *d_Dspin, double hyb, const double *d_Q, const double *s, int K,
                                 double *d_grad, int rank, int nranks, void *stream)
{
    if (check_terms("mi_grad_eri_pairs", PAIR_NAMES, d_Q, s, K, 136)) return -1;
    return grad_eri_run(c, d_D, d_Dspin, hyb, d_Q, s, K, d_grad, rank, nranks, stream);
}

// The pass of mi_grad_eri_pairs with signed exchange-type terms as well: the gradient, at fixed matrices, of
//   1/2 (D|D) - hyb/4 [tr(D K[D]) + tr(M K[M])] + 1/2 sum_k s_k (Q^k|Q^k) + sum_m t_m sum_ijkl (ik|jl) R^m_ij R^m_kl.
// Every quartet's two-particle density gains sum_m t_m (R^m_ac R^m_bd + R^m_ad R^m_bc); each R^m is symmetric (sym[m] = +1) or
// antisymmetric (-1) (xpair_term: the same element formula serves both).  Kx = 0 is mi_grad_eri_pairs.
extern "C" int mi_grad_eri_xpairs(mi_ctx *c, const double *d_D, const double *d_Dspin, double hyb, const double *d_Q, const double *s, int K,
                                  const double *d_R, const double *t, const int *sym, int Kx, double *d_grad, int rank, int nranks, void *stream)
{
    if (check_terms("mi_grad_eri_xpairs", XPAIR_NAMES, sym ? d_R : nullptr, t, Kx, 8, sym)) return -1;   // (a null sym is a null argument too)
    if (check_terms("mi_grad_eri_xpairs", PAIR_NAMES, d_Q, s, K, 136)) return -1;
    return grad_eri_run(c, d_D, d_Dspin, hyb, d_Q, s, K, d_grad, rank, nranks, stream, d_R, t, Kx);
}

extern "C" int mi_grad_eri(mi_ctx *c, const double *d_D, double hyb, double *d_grad, void *stream)
{
    return c ? mi_grad_eri_sharded(c, d_D, nullptr, hyb, d_grad, c->rank, c->nranks, stream) : fail("mi_grad_eri: null argument");
}

extern "C" int mi_grad_eri_spin(mi_ctx *c, const double *d_D, const double *d_Dspin, double hyb, double *d_grad, void *stream)
{
    return c ? mi_grad_eri_sharded(c, d_D, d_Dspin, hyb, d_grad, c->rank, c->nranks, stream) : fail("mi_grad_eri: null argument");
}

// =================================================================================================
// Nuclear gradient of the density-fitted two-electron energy (`mf.density_fit().nuc_grad_method()`
// is PySCF idiom [MEM], the reference never calls it):
//
//   grad_X += sum_{ab,P} Z3[a][b][P] d/dX (ab|P)  +  sum_{PQ} Z2[P][Q] d/dX (P|Q)
//
// Z3 (symmetric in ab) and Z2 (symmetric) are the three- and two-index densities the host forms from the fitted tensor
// (python/mi355scf/df.py: Z3 = c_P D_ab - hyb/2 Gamma^P_ab, Z2 = -c c^T / 2 + hyb/4 C.Gamma).  The derivative integrals go
// through the SAME Rys kernel and contraction kernel as the four-centre gradient: the differentiated pair is an orbital pair
// (either shell: two launches) or an auxiliary "pair" (P, unit function), its (l+1) / (l-1) variants carry 2 alpha c / c, the
// ket is an auxiliary pair, and the force on the auxiliary centre follows from translational invariance (minus the force on
// the differentiated shell).  Batches are dealt round-robin to `nranks` callers; the caller sums the partial gradients.
// =================================================================================================
extern "C" int mi_df_grad(mi_ctx *c, mi_ctx *aux, const double *d_Z3, const double *d_Z2, double *d_grad, int rank, int nranks, void *stream)
{
    if (!c || !aux || !d_grad) return fail("mi_df_grad: null argument");
    if (c->opt_omega != 0.0 || c->eri_omega != 0.0 || aux->opt_omega != 0.0 || aux->eri_omega != 0.0)
        return fail("mi_df_grad: no derivative integrals for a long-range (omega != 0) context");
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail("mi_df_grad: bad rank/nranks");
    if (aux->nbas < 2) return fail("mi_df_grad: the auxiliary context needs at least one function plus the unit shell");
    if (aux->natm != c->natm) return fail("mi_df_grad: orbital and auxiliary contexts must share the atom list");
    const ShellH &U = aux->shells.back();
    if (U.l != 0 || U.nprim != 1 || U.exps[0] != 0.0) return fail("mi_df_grad: the last auxiliary shell must be the unit s function (exponent 0)");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    const int naux = aux->nao - 1, unit_ao = aux->nao - 1, nP = aux->nbas - 1, nao = c->nao;
    std::vector<double> prim, Mbuf;
    // variant records: orbital pairs [class][orientation][l+1 | l-1] (parallel arrays), auxiliary pairs [l][l+1 | l-1]; plain auxiliary kets [l]
    std::vector<PairRec> orb[NPC][2][2], axv[LMAX + 1][2], axk[LMAX + 1];
    VariantRecords V(0, 0);
    if (d_Z3)
        for (int A = 0; A < c->nbas; A++)
            for (int B = 0; B <= A; B++) {
                int si = A, sj = B;
                if (c->shells[si].l < c->shells[sj].l) std::swap(si, sj);
                const ShellH &I = c->shells[si], &J = c->shells[sj];
                if (count_prim_pairs(I, J) == 0) continue;
                const int q = pc_index(I.l, J.l);
                for (int o = 0; o < 2; o++) {
                    const ShellH &F = o == 0 ? I : J, &S = o == 0 ? J : I;
                    PairRec R[2];
                    V.add_pair(F, S, o == 0 ? si : sj, o == 0 ? sj : si, F.ao_nat, S.ao_nat, R);
                    for (int sg = 0; sg < 2; sg++) orb[q][o][sg].push_back(R[sg]);
                }
            }
    for (int Pn = 0; Pn < nP; Pn++) {
        const ShellH &S = aux->shells[Pn];
        PairRec Rv[2];
        V.add_pair(S, U, Pn, aux->nbas - 1, S.ao_nat, unit_ao, Rv);
        for (int sg = 0; sg < 2; sg++) axv[S.l][sg].push_back(Rv[sg]);
        PairRec R{Pn, aux->nbas - 1, S.ao_nat, unit_ao, (int)V.prim_end, S.nprim, (int)V.m_end, 0};     // plain ket record (filled below)
        V.prim_end += S.nprim;
        V.m_end += (size_t)(2 * S.l + 1) * ncart(S.l);
        axk[S.l].push_back(R);
    }
    if (V.m_end > (size_t)INT32_MAX || V.prim_end > (size_t)INT32_MAX) return fail("mi_df_grad: record buffers exceed 2^31 entries");
    prim.resize(V.prim_end * 8);
    Mbuf.resize(V.m_end);
    V.fill(prim, Mbuf);
    {
        const std::vector<std::vector<double>> c2s = c2s_tables();
        for (int l = 0; l <= LMAX; l++)
            for (PairRec &R : axk[l]) {
                const ShellH &S = aux->shells[R.sh_i];
                write_aux_prims(S, U, prim.data() + (size_t)R.prim_off * 8);
                double AB[3] = {0.0, 0.0, 0.0};
                build_M(S.l, 0, AB, c2s[S.l], c2s[0], Mbuf.data() + R.m_off);
            }
    }
    std::vector<int> atom_o(c->nbas), atom_a(aux->nbas);
    for (int i = 0; i < c->nbas; i++) atom_o[i] = c->shells[i].atom;
    for (int i = 0; i < aux->nbas; i++) atom_a[i] = aux->shells[i].atom;
    DevBuf<double> d_prim, d_M, d_wp, d_wm, d_gcopies;
    DevBuf<uint32_t> d_comp_p, d_comp_m;
    DevBuf<int64_t> d_prefix;
    DevBuf<int> d_atom_o, d_atom_a;
    DevBuf<PairRec> d_orb[NPC][2][2], d_axv[LMAX + 1][2], d_axk[LMAX + 1];
    if (d_prim.upload(prim) || d_M.upload(Mbuf) || d_atom_o.upload(atom_o) || d_atom_a.upload(atom_a)) return -1;
    for (int q = 0; q < NPC; q++)
        for (int o = 0; o < 2; o++)
            for (int sg = 0; sg < 2; sg++)
                if (!orb[q][o][sg].empty() && d_orb[q][o][sg].upload(orb[q][o][sg])) return -1;
    for (int l = 0; l <= LMAX; l++) {
        for (int sg = 0; sg < 2; sg++)
            if (!axv[l][sg].empty() && d_axv[l][sg].upload(axv[l][sg])) return -1;
        if (!axk[l].empty() && d_axk[l].upload(axk[l])) return -1;
    }
    const size_t WORK_DOUBLES = (size_t)32 << 20;
    HIPCHK(d_wp.alloc(WORK_DOUBLES));
    HIPCHK(d_wm.alloc(WORK_DOUBLES));
    HIPCHK(d_comp_p.alloc(COMP_CAP));
    HIPCHK(d_comp_m.alloc(COMP_CAP));
    const int natm3 = c->natm * 3;
    HIPCHK(d_gcopies.alloc((size_t)GRAD_COPIES * natm3));
    HIPCHK(hipMemsetAsync(d_gcopies, 0, sizeof(double) * (size_t)GRAD_COPIES * natm3, st));
    int64_t batch_counter = 0;
    const bool dbg = getenv("MI355_DEBUG") != nullptr;
    // one pass: differentiated pairs `dp`/`dm` (l1 first, l2 second) against the auxiliary kets of angular momentum lk
    auto run = [&](const PairRec *dp, const PairRec *dm, int nbra, int l1, int l2, int lk, const double *Z, int64_t zs_i, int64_t zs_j,
                   const int *bra_atom, double w0) -> int {
        const int nket = (int)axk[lk].size();
        if (nbra == 0 || nket == 0) return 0;
        const auto tr0 = std::chrono::steady_clock::now();
        std::vector<int64_t> prefix;
        const int64_t ntask = dense_prefix(nbra, nket, prefix);
        if (prefix_to_device(prefix, d_prefix, st)) return -1;
        const bool has_m = l1 >= 1;
        if (upload_comp_table(l1 + 1, l2, lk, 0, d_comp_p, st)) return -1;
        if (has_m && upload_comp_table(l1 - 1, l2, lk, 0, d_comp_m, st)) return -1;
        EriArgs Ep = eri_class_args(c, l1 + 1, l2, lk, 0, dp, d_axk[lk], d_prim, d_prefix, nbra, d_comp_p, d_wp), Em{};
        if (has_m) Em = eri_class_args(c, l1 - 1, l2, lk, 0, dm, d_axk[lk], d_prim, d_prefix, nbra, d_comp_m, d_wm);
        GradXfArgs X{};
        X.dplus = dp; X.dminus = has_m ? dm : nullptr; X.ket = d_axk[lk]; X.Mbuf = d_M; X.prefix = d_prefix; X.nbra = nbra;
        X.ne_p = ne_of(l1 + 1, l2); X.ne_m = has_m ? ne_of(l1 - 1, l2) : 0; X.nf = ncart(lk);
        X.ns1 = 2 * l1 + 1; X.ns2 = 2 * l2 + 1; X.nscd = 2 * lk + 1; X.nsd = 1;
        X.work_p = d_wp; X.work_m = d_wm; X.ncomp_p = Ep.ncomp; X.ncomp_m = has_m ? Em.ncomp : 0;
        X.shell_atom = bra_atom; X.ket_atom = d_atom_a; X.grad = d_gcopies; X.natm3 = natm3;
        X.Z = Z; X.zs_i = zs_i; X.zs_j = zs_j; X.w0 = w0;
        const size_t shm = sizeof(double) * ((size_t)X.ne_p * X.nf + (size_t)X.ne_m * X.nf + (size_t)X.ns1 * X.ns2 * (X.nf + X.nscd));
        if (shm > 160 * 1024) return fail("gradient contraction needs %zu bytes of LDS", shm);
        int64_t per = std::min<int64_t>((int64_t)(WORK_DOUBLES / Ep.ncomp), (int64_t)1 << 22);
        if (nranks > 1) per = std::min<int64_t>(per, std::max<int64_t>(1024, ntask / (8 * nranks)));
        if (c->opt_df_batch_max > 0) per = std::min<int64_t>(per, c->opt_df_batch_max);
        for (int64_t t0 = 0; t0 < ntask; t0 += per) {
            if ((int)((batch_counter++) % nranks) != rank) continue;
            const int nb = (int)std::min<int64_t>(per, ntask - t0);
            Ep.t0 = t0; Ep.ntask = nb;
            if (launch_eri(c, Ep, nb, st)) return -1;
            if (has_m) { Em.t0 = t0; Em.ntask = nb; if (launch_eri(c, Em, nb, st)) return -1; }
            X.t0 = t0; X.nbatch = nb;
            if (launch_grad_contract(true, X, has_m, nb, shm, st)) return -1;
        }
        HIPCHK(hipStreamSynchronize(st));
        if (dbg)
            fprintf(stderr, "[mi355] df_grad (%d %d|%d): %ld tasks, %.3f s\n", l1, l2, lk, (long)ntask,
                    std::chrono::duration<double>(std::chrono::steady_clock::now() - tr0).count());
        return 0;
    };
    int rc = 0;
    if (d_Z3)   // sum_ab over canonical shell pairs: weight 2 (1 on the diagonal, halved in the kernel), both orientations
        for (int la = 0; la <= LMAX && !rc; la++)
            for (int lb = 0; lb <= la && !rc; lb++)
                for (int o = 0; o < 2 && !rc; o++)
                    for (int lk = 0; lk <= LMAX && !rc; lk++) {
                        const int q = pc_index(la, lb);
                        rc = run(d_orb[q][o][0], d_orb[q][o][1], (int)orb[q][o][0].size(), o == 0 ? la : lb, o == 0 ? lb : la, lk, d_Z3,
                                 (int64_t)nao * naux, (int64_t)naux, d_atom_o, 2.0);
                    }
    if (d_Z2)   // every ordered pair (P, Q): +v on the centre of P, -v on the centre of Q
        for (int lp = 0; lp <= LMAX && !rc; lp++)
            for (int lk = 0; lk <= LMAX && !rc; lk++)
                rc = run(d_axv[lp][0], d_axv[lp][1], (int)axv[lp][0].size(), lp, 0, lk, d_Z2, (int64_t)naux, 0, d_atom_a, 1.0);
    if (!rc) {
        hipLaunchKernelGGL(grad_reduce_copies_kernel, dim3((natm3 + 63) / 64), dim3(64), 0, st, d_gcopies.get(), natm3, d_grad);
        HIPCHK(hipStreamSynchronize(st));
    }
    return rc;
}

// =================================================================================================
// Fused SP2 step for small matrices (N <= 512): ONE launch per purification step instead of a rocBLAS
// DGEMM (launch-latency bound at 10 us for N=114) plus an update kernel.
//   Xc  = first ? Xp : ( |tr X2p - N| < |2 tr Xp - tr X2p - N| ? X2p : 2 Xp - X2p )   (formed on the fly)
//   X2c = Xc * Xc^T (X is symmetric), 16x16 output tile per workgroup on v_mfma_f64_16x16x4_f64,
//   K split over the 4 waves of the workgroup, row panels staged in LDS; every diagonal workgroup b writes its share of
//   tr Xc, tr X2c to trc[2b], trc[2b+1] and the next launch adds the SP2_TRS slots in index order for its branch decision
//   (no atomics: bit-identical on every rank of a sharded run).
// =================================================================================================
#define SP2_TRS 32 /* trace slots per step = max diagonal workgroups (N <= 512) */
// LDS row padding of the panels (doubles).  The MFMA operand read is "16 rows x 4 consecutive k" per wave; a row stride of
// 2 (mod 32) doubles = 4 banks (mod 64) puts the 32 lanes of a half wave on 64 distinct banks, where +4 makes rows r and r + 8
// share banks.  Measured (round 2): no difference in kernel time for either padding, here (7.3-7.4 us per pass) or in xc_vmat
// (518 vs 543 us on boxes whose J/K pass differed by more) -- the operand reads are not what bounds these kernels.
#define SP2_PAD 2
// MAXM = 16-column groups a thread loads per panel row in one batch: all 4 x MAXM loads of a thread are in flight together
// (one memory round trip for kpad <= 16 MAXM; larger matrices take two batches).  Thread t owns row t/16 and columns
// t%16 + 16 m of both panels: no integer division, 128-byte segments per row and instruction.
// PLAN = true: the step is a quadratic fixed by the host, Xc = ca X2p + cb Xp + cc I (no dependence on the previous
// launch's traces; `first`: Xc = cb Xp + cc I, the affine map of the Fock matrix); PLAN = false: trace-correcting SP2.
struct Sp2Coef { double a, b, c; double out_scale; };   // out_scale: factor on the stored X (0 = 1); the traces stay those of X
template <int MAXM, bool PLAN>
__global__ __launch_bounds__(256) void sp2_fused_kernel(const double *__restrict__ Xp, const double *__restrict__ X2p,
                                                        const double *__restrict__ trp, int first, int n, int kpad, double target,
                                                        double *__restrict__ Xc, double *__restrict__ X2c, double *__restrict__ trc,
                                                        Sp2Coef cf)
{
    extern __shared__ double lds[];
    double *Pa = lds;                       // [16][kpad+SP2_PAD]  rows i0..i0+15 of Xc
    double *Pb = lds + 16 * (kpad + SP2_PAD);     // [16][kpad+SP2_PAD]  rows j0..j0+15 of Xc
    double *red = Pb + 16 * (kpad + SP2_PAD);     // [4][256]  (its first 64 doubles also stage the partial traces)
    const int ldp = kpad + SP2_PAD;
    // X and X^2 are symmetric: only the tiles (I >= J) are computed (grid = nb(nb+1)/2 workgroups -- 153 for N = 264, one round
    // on 256 CUs instead of 289 in two) and every off-diagonal tile is stored with its mirror image.  The mirrored values are
    // bit-identical to what the (J, I) workgroup used to compute (same products, same k order).
    int bI = (int)((sqrt(8.0 * blockIdx.x + 1.0) - 1.0) * 0.5);
    while ((bI + 1) * (bI + 2) / 2 <= (int)blockIdx.x) bI++;
    while (bI * (bI + 1) / 2 > (int)blockIdx.x) bI--;
    const int bJ = (int)blockIdx.x - bI * (bI + 1) / 2;
    const int i0 = bI * 16, j0 = bJ * 16;
    const int t = threadIdx.x, r = t >> 4, c = t & 15;
    const int nbd = (n + 15) / 16;
    // partial traces of the previous launch: ONE coalesced load (thread b <- slot b), staged in LDS and added in index order
    // by everybody -- issued together with the panel loads so that the latencies overlap
    double trv = 0.0;
    if (!PLAN && !first && t < 2 * nbd) trv = trp[t];
    const bool ra = i0 + r < n, rb = j0 + r < n;
    const double *xa_row = Xp + (size_t)(i0 + r) * n, *xb_row = Xp + (size_t)(j0 + r) * n;
    const double *ya_row = X2p + (size_t)(i0 + r) * n, *yb_row = X2p + (size_t)(j0 + r) * n;
    const int mtot = kpad >> 4;
    bool sq = false;
    for (int m0 = 0; m0 < mtot; m0 += MAXM) {
        double xa[MAXM], ya[MAXM], xb[MAXM], yb[MAXM];
#pragma unroll
        for (int u = 0; u < MAXM; u++) {
            const int k = c + 16 * (m0 + u);
            const bool in = (m0 + u < mtot) && k < n;
            xa[u] = (in && ra) ? xa_row[k] : 0.0;
            xb[u] = (in && rb) ? xb_row[k] : 0.0;
            ya[u] = (in && ra && !first) ? ya_row[k] : 0.0;
            yb[u] = (in && rb && !first) ? yb_row[k] : 0.0;
        }
        if (!PLAN && m0 == 0 && !first) {
            red[t] = trv;
            __syncthreads();
            double tx = 0.0, tx2 = 0.0;
            for (int b = 0; b < nbd; b++) { tx += red[2 * b]; tx2 += red[2 * b + 1]; }
            sq = fabs(tx2 - target) < fabs(2.0 * tx - tx2 - target);
            __syncthreads();                 // `red` is reused by the K-split reduction below
        }
#pragma unroll
        for (int u = 0; u < MAXM; u++) {
            const int k = c + 16 * (m0 + u);
            if (m0 + u < mtot) {
                if (PLAN) {   // zero padding (k >= n, rows >= n) must stay zero: the identity term only on real diagonal elements
                    const double da = (ra && k < n && k == i0 + r) ? cf.c : 0.0, db = (rb && k < n && k == j0 + r) ? cf.c : 0.0;
                    Pa[r * ldp + k] = fma(cf.a, ya[u], fma(cf.b, xa[u], da));
                    Pb[r * ldp + k] = fma(cf.a, yb[u], fma(cf.b, xb[u], db));
                } else {
                    Pa[r * ldp + k] = first ? xa[u] : (sq ? ya[u] : 2.0 * xa[u] - ya[u]);
                    Pb[r * ldp + k] = first ? xb[u] : (sq ? yb[u] : 2.0 * xb[u] - yb[u]);
                }
            }
        }
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int kq = kpad / 4; // k-range per wave (multiple of 4)
    d4_t acc = {0.0, 0.0, 0.0, 0.0};
    const double *pa = Pa + (lane & 15) * ldp + wave * kq + (lane >> 4);
    const double *pb = Pb + (lane & 15) * ldp + wave * kq + (lane >> 4);
    for (int k = 0; k < kq; k += 4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[k], pb[k], acc, 0, 0, 0);
#pragma unroll
    for (int q = 0; q < 4; q++) red[wave * 256 + q * 64 + lane] = acc[q];
    __syncthreads();
    if (wave == 0) {
        double tr2 = 0.0, tr1 = 0.0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            double v = (red[q * 64 + lane] + red[256 + q * 64 + lane]) + (red[512 + q * 64 + lane] + red[768 + q * 64 + lane]);
            int col = lane & 15, row = (lane >> 4) + 4 * q; // f64 MFMA C/D layout
            int gi = i0 + row, gj = j0 + col;
            if (gi < n && gj < n) {
                X2c[(size_t)gi * n + gj] = v;
                double xc = Pa[row * ldp + gj];
                const double osc = (PLAN && cf.out_scale != 0.0) ? cf.out_scale : 1.0;
                Xc[(size_t)gi * n + gj] = osc * xc;
                if (bI != bJ) {
                    X2c[(size_t)gj * n + gi] = v;
                    Xc[(size_t)gj * n + gi] = osc * Pb[col * ldp + gi];
                }
                if (gi == gj) { tr2 += v; tr1 += xc; }
            }
        }
        if (bI == bJ) {
            for (int o = 32; o > 0; o >>= 1) { tr1 += __shfl_xor(tr1, o); tr2 += __shfl_xor(tr2, o); }
            if (lane == 0) { trc[2 * bI] = tr1; trc[2 * bI + 1] = tr2; }
        }
    }
}

// Planned purification, one matrix per pass: the polynomial of the NEXT pass is applied in the epilogue of this one,
//   pass k:  reads X_k (pass 0: b_in F + c_in I formed while loading), computes the tile of X_k^2 and the traces of X_k, X_k^2,
//            writes X_{k+1} = a X_k^2 + b X_k + c I   (last pass: a = c = 0, b = out_scale: the result itself),
// so a pass loads two row panels and stores one tile where the two-matrix version loaded four and stored two.  Same triangular
// grid, same mirror stores, same MFMA/K-split order as sp2_fused_kernel: the traces are bit-identical to that kernel's.
__device__ inline void sp2_tile_of_block(int b, int &bI, int &bJ)
{
    bI = (int)((sqrt(8.0 * b + 1.0) - 1.0) * 0.5);
    while ((bI + 1) * (bI + 2) / 2 <= b) bI++;
    while (bI * (bI + 1) / 2 > b) bI--;
    bJ = b - bI * (bI + 1) / 2;
}
// one pass for the tile (bI, bJ)
template <int MAXM>
__device__ __forceinline__ void sp2_plan_pass(const double *Xin, int n, int kpad, double b_in, double c_in, double *Xout, double *trc,
                                              Sp2Coef nx, int bI, int bJ, double *lds)
{
    double *Pa = lds;                       // [16][kpad+SP2_PAD]  rows i0..i0+15 of X_k
    double *Pb = lds + 16 * (kpad + SP2_PAD);     // [16][kpad+SP2_PAD]  rows j0..j0+15 of X_k
    double *red = Pb + 16 * (kpad + SP2_PAD);     // [4][256]
    const int ldp = kpad + SP2_PAD;
    const int i0 = bI * 16, j0 = bJ * 16;
    const int t = threadIdx.x, r = t >> 4, c = t & 15;
    const bool ra = i0 + r < n, rb = j0 + r < n;
    const double *xa_row = Xin + (size_t)(i0 + r) * n, *xb_row = Xin + (size_t)(j0 + r) * n;
    const int mtot = kpad >> 4;
    for (int m0 = 0; m0 < mtot; m0 += MAXM) {
        double xa[MAXM], xb[MAXM];
#pragma unroll
        for (int u = 0; u < MAXM; u++) {
            const int k = c + 16 * (m0 + u);
            const bool in = (m0 + u < mtot) && k < n;
            xa[u] = (in && ra) ? xa_row[k] : 0.0;
            xb[u] = (in && (bI != bJ) && rb) ? xb_row[k] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < MAXM; u++) {
            const int k = c + 16 * (m0 + u);
            if (m0 + u < mtot) {   // zero padding (k >= n, rows >= n) must stay zero: the identity term only on real diagonal elements
                const double da = (ra && k < n && k == i0 + r) ? c_in : 0.0, db = (rb && k < n && k == j0 + r) ? c_in : 0.0;
                const double va = fma(b_in, xa[u], da);
                Pa[r * ldp + k] = va;
                Pb[r * ldp + k] = (bI != bJ) ? fma(b_in, xb[u], db) : va;
            }
        }
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int kq = kpad / 4; // k-range per wave (multiple of 4)
    d4_t acc = {0.0, 0.0, 0.0, 0.0};
    const double *pa = Pa + (lane & 15) * ldp + wave * kq + (lane >> 4);
    const double *pb = Pb + (lane & 15) * ldp + wave * kq + (lane >> 4);
    for (int k = 0; k < kq; k += 4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[k], pb[k], acc, 0, 0, 0);
#pragma unroll
    for (int q = 0; q < 4; q++) red[wave * 256 + q * 64 + lane] = acc[q];
    __syncthreads();
    if (wave == 0) {
        double tr2 = 0.0, tr1 = 0.0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            double v = (red[q * 64 + lane] + red[256 + q * 64 + lane]) + (red[512 + q * 64 + lane] + red[768 + q * 64 + lane]);
            int col = lane & 15, row = (lane >> 4) + 4 * q; // f64 MFMA C/D layout
            int gi = i0 + row, gj = j0 + col;
            if (gi < n && gj < n) {
                const double xc = Pa[row * ldp + gj];
                const double dg = (gi == gj) ? nx.c : 0.0;
                Xout[(size_t)gi * n + gj] = fma(nx.a, v, fma(nx.b, xc, dg));
                if (bI != bJ) Xout[(size_t)gj * n + gi] = fma(nx.a, v, nx.b * Pb[col * ldp + gi]);
                if (gi == gj) { tr2 += v; tr1 += xc; }
            }
        }
        if (bI == bJ) {
            for (int o = 32; o > 0; o >>= 1) { tr1 += __shfl_xor(tr1, o); tr2 += __shfl_xor(tr2, o); }
            if (lane == 0) { trc[2 * bI] = tr1; trc[2 * bI + 1] = tr2; }
        }
    }
}
template <int MAXM>
__global__ __launch_bounds__(256) void sp2_plan_kernel(const double *__restrict__ Xin, int n, int kpad, double b_in, double c_in,
                                                       double *__restrict__ Xout, double *__restrict__ trc, Sp2Coef nx)
{
    extern __shared__ double lds[];
    int bI, bJ;
    sp2_tile_of_block((int)blockIdx.x, bI, bJ);
    sp2_plan_pass<MAXM>(Xin, n, kpad, b_in, c_in, Xout, trc, nx, bI, bJ, lds);
}

// The same planned pass with the MFMA operands loaded straight into registers (option sp2_direct, N <= 16 MAXS).
// X_k is symmetric, so row i of X_k is also its column i: the A operand of v_mfma_f64_16x16x4f64 (lane l: row i0 + l % 16,
// k = 4 s + l / 16 of step s) is read as X_k[k][i0 + l % 16], and each load instruction of a wave covers four whole 128-byte
// row segments -- the coalescing of the LDS-staged panel loads without the staging, its barrier and the dependent LDS reads in
// front of every MFMA.  Each wave keeps the K-quarter of sp2_plan_kernel (k = wave kq + 4 s + l / 16) on two interleaved
// accumulators; LDS holds only the 4-way K reduction, and the epilogue is spread over the four waves (wave w: rows 4w..4w+3
// of the tile, the C/D rows of the q = w register).  The element and mirror of X_k that the next-pass polynomial needs are
// loaded with the operands.  Summation order fixed per build, no atomics: the traces repeat bit for bit from run to run.
// Pass 0 of a Fock matrix that is symmetric only to rounding reads its columns where sp2_plan_kernel read its rows.
template <int MAXS>
__global__ __launch_bounds__(256) void sp2_direct_kernel(const double *__restrict__ Xin, int n, int S, double b_in, double c_in,
                                                         double *__restrict__ Xout, double *__restrict__ trc, Sp2Coef nx)
{
    __shared__ double red[4 * 256];
    __shared__ double trs[4][2];
    int bI, bJ;
    sp2_tile_of_block((int)blockIdx.x, bI, bJ);
    const bool diag = bI == bJ;
    const int i0 = bI * 16, j0 = bJ * 16;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, col = lane & 15, g = lane >> 4;
    const int ia = i0 + col, jb = j0 + col;
    const int kw = wave * 4 * S + g;            // k of step s: kw + 4 s
    // epilogue element (gi, gj) of this lane and the input elements the polynomial reads, issued with the operand loads
    const int gi = i0 + g + 4 * wave, gj = j0 + col;
    const bool own = gi < n && gj < n;
    const int ci = min(gi, n - 1), cj = min(gj, n - 1);
    const double xt = Xin[(size_t)ci * n + cj], xm = Xin[(size_t)cj * n + ci];
    // unconditional loads from clamped (in-bounds) addresses, out-of-range values dropped below: no branch around every load
    const int ca = min(ia, n - 1), cb = min(jb, n - 1);
    double a[MAXS], b[MAXS];
#pragma unroll
    for (int s = 0; s < MAXS; s++) {
        const size_t row = (size_t)min(kw + 4 * s, n - 1) * n;
        a[s] = Xin[row + ca];
        b[s] = Xin[row + cb];
    }
    // pass 0: X_0 = b_in F + c_in I on the real elements; the zero padding stays zero
#pragma unroll
    for (int s = 0; s < MAXS; s++) {
        const int k = kw + 4 * s;
        const bool in = s < S && k < n;
        a[s] = (in && ia < n) ? fma(b_in, a[s], k == ia ? c_in : 0.0) : 0.0;
        b[s] = diag ? a[s] : ((in && jb < n) ? fma(b_in, b[s], k == jb ? c_in : 0.0) : 0.0);
    }
    d4_t acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < MAXS; s += 2) {
        if (s < S) acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b[s], acc0, 0, 0, 0);
        if (s + 1 < MAXS && s + 1 < S) acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s + 1], b[s + 1], acc1, 0, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < 4; q++) red[wave * 256 + q * 64 + lane] = acc0[q] + acc1[q];
    __syncthreads();
    const int e = wave * 64 + lane;             // C/D register q = wave: row g + 4 wave, column col
    const double v = (red[e] + red[256 + e]) + (red[512 + e] + red[768 + e]);
    double tr1 = 0.0, tr2 = 0.0;
    if (own) {
        const double xc = fma(b_in, xt, gi == gj ? c_in : 0.0);
        Xout[(size_t)gi * n + gj] = fma(nx.a, v, fma(nx.b, xc, gi == gj ? nx.c : 0.0));
        if (!diag) Xout[(size_t)gj * n + gi] = fma(nx.a, v, nx.b * fma(b_in, xm, 0.0));
        if (gi == gj) { tr1 = xc; tr2 = v; }
    }
    if (diag) {   // uniform over the workgroup
        for (int o = 32; o > 0; o >>= 1) { tr1 += __shfl_xor(tr1, o); tr2 += __shfl_xor(tr2, o); }
        if (lane == 0) { trs[wave][0] = tr1; trs[wave][1] = tr2; }
        __syncthreads();
        if (threadIdx.x == 0) {
            trc[2 * bI] = (trs[0][0] + trs[1][0]) + (trs[2][0] + trs[3][0]);
            trc[2 * bI + 1] = (trs[0][1] + trs[1][1]) + (trs[2][1] + trs[3][1]);
        }
    }
}
#define SP2_DIRECT_MAXS 20   /* N <= 320 */
typedef void (*sp2_direct_fn)(const double *, int, int, double, double, double *, double *, Sp2Coef);
static sp2_direct_fn sp2_direct_for(int S)
{
    if (S <= 8) return sp2_direct_kernel<8>;
    if (S <= 12) return sp2_direct_kernel<12>;
    if (S <= 16) return sp2_direct_kernel<16>;
    return sp2_direct_kernel<SP2_DIRECT_MAXS>;
}

typedef void (*sp2_plan_fn)(const double *, int, int, double, double, double *, double *, Sp2Coef);

static sp2_plan_fn sp2_plan_for(int kpad)
{
    const int m = kpad >> 4;
    if (m <= 8) return sp2_plan_kernel<8>;
    if (m <= 12) return sp2_plan_kernel<12>;
    if (m <= 16) return sp2_plan_kernel<16>;
    if (m <= 20) return sp2_plan_kernel<20>;
    return sp2_plan_kernel<16>; // two batches
}

typedef void (*sp2_fused_fn)(const double *, const double *, const double *, int, int, int, double, double *, double *, double *, Sp2Coef);
template <bool PLAN> static sp2_fused_fn sp2_fused_for_t(int kpad)
{
    const int m = kpad >> 4;
    if (m <= 8) return sp2_fused_kernel<8, PLAN>;
    if (m <= 12) return sp2_fused_kernel<12, PLAN>;
    if (m <= 16) return sp2_fused_kernel<16, PLAN>;
    if (m <= 20) return sp2_fused_kernel<20, PLAN>;
    return sp2_fused_kernel<16, PLAN>; // two batches
}
static sp2_fused_fn sp2_fused_for(int kpad) { return sp2_fused_for_t<false>(kpad); }

// d_X (in/out), d_X2 (in if have_x2, out), d_work: 2*n*n doubles, d_tr: (nit+2)*2*SP2_TRS doubles (device).
// On return d_X = X_nit, d_X2 = X_nit^2 and d_tr_out points at the 2*ceil(n/16) partial traces {tr X, tr X^2} interleaved
// (device pointer into d_tr; the caller adds them in index order).
extern "C" int mi_sp2_iterate(mi_ctx *c, double *d_X, double *d_X2, int nit, double n_occ, int have_x2, double *d_work,
                              double *d_tr, double **d_tr_out, void *stream)
{
    if (!c || !d_X || !d_X2 || !d_work || !d_tr || !d_tr_out || nit < 0) return fail("mi_sp2_iterate: bad argument");
    const int n = c->nao;
    if (n > 512) return fail("mi_sp2_iterate: fused path is for N <= 512");
    hipStream_t st = (hipStream_t)stream;
    const int kpad = ((n + 15) / 16) * 16;
    const size_t shm = sizeof(double) * (2 * 16 * (kpad + SP2_PAD) + 4 * 256);
    const int nb = (n + 15) / 16;
    dim3 grid(nb * (nb + 1) / 2), block(256);
    const size_t nn = (size_t)n * n;
    (void)have_x2; // X^2 and the traces of the incoming X are always (re)derived by the first pass
    constexpr int TS = 2 * SP2_TRS;
    const sp2_fused_fn sp2_fused_kernel = sp2_fused_for(kpad);
    double *cur_x = d_X, *cur_x2 = d_X2, *nxt_x = d_work, *nxt_x2 = d_work + nn;
    int slot = 0;
    hipLaunchKernelGGL(sp2_fused_kernel, grid, block, shm, st, cur_x, cur_x2, d_tr, 1, n, kpad, n_occ, nxt_x, nxt_x2, d_tr + TS * slot, Sp2Coef{});
    std::swap(cur_x, nxt_x); std::swap(cur_x2, nxt_x2);
    for (int it = 0; it < nit; it++) {
        hipLaunchKernelGGL(sp2_fused_kernel, grid, block, shm, st, cur_x, cur_x2, d_tr + TS * slot, 0, n, kpad, n_occ, nxt_x, nxt_x2,
                           d_tr + TS * (slot + 1), Sp2Coef{});
        slot++;
        std::swap(cur_x, nxt_x); std::swap(cur_x2, nxt_x2);
    }
    HIPCHK(hipGetLastError());
    if (cur_x != d_X) {
        HIPCHK(hipMemcpyAsync(d_X, cur_x, sizeof(double) * nn, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(d_X2, cur_x2, sizeof(double) * nn, hipMemcpyDeviceToDevice, st));
    }
    *d_tr_out = d_tr + TS * slot;
    return 0;
}

// Same passes on two caller-owned [X | X2] buffers (2 n^2 doubles each, X0 in d_A[0 : n^2]) WITHOUT the final copy:
// *d_res tells which of the two buffers holds {X_nit, X_nit^2}.
extern "C" int mi_sp2_iterate_pingpong(mi_ctx *c, double *d_A, double *d_B, int nit, double n_occ, double *d_tr, double **d_tr_out,
                                       double **d_res, void *stream)
{
    if (!c || !d_A || !d_B || !d_tr || !d_tr_out || !d_res || nit < 0) return fail("mi_sp2_iterate_pingpong: bad argument");
    const int n = c->nao;
    if (n > 512) return fail("mi_sp2_iterate_pingpong: fused path is for N <= 512");
    hipStream_t st = (hipStream_t)stream;
    const int kpad = ((n + 15) / 16) * 16;
    const size_t shm = sizeof(double) * (2 * 16 * (kpad + SP2_PAD) + 4 * 256);
    const int nb = (n + 15) / 16;
    dim3 grid(nb * (nb + 1) / 2), block(256);
    const size_t nn = (size_t)n * n;
    constexpr int TS = 2 * SP2_TRS;
    const sp2_fused_fn sp2_fused_kernel = sp2_fused_for(kpad);
    double *cur = d_A, *nxt = d_B;
    hipLaunchKernelGGL(sp2_fused_kernel, grid, block, shm, st, cur, cur + nn, d_tr, 1, n, kpad, n_occ, nxt, nxt + nn, d_tr, Sp2Coef{});
    std::swap(cur, nxt);
    for (int it = 0; it < nit; it++) {
        hipLaunchKernelGGL(sp2_fused_kernel, grid, block, shm, st, cur, cur + nn, d_tr + TS * it, 0, n, kpad, n_occ, nxt, nxt + nn,
                           d_tr + TS * (it + 1), Sp2Coef{});
        std::swap(cur, nxt);
    }
    HIPCHK(hipGetLastError());
    *d_tr_out = d_tr + TS * nit;
    *d_res = cur;
    return 0;
}

// Planned purification (round 2): the host knows inner bounds of the HOMO / LUMO and outer bounds of the spectrum (from the
// last diagonalisation) and fixes the whole sequence of quadratics in advance -- each step folds one band of the spectrum
// about a point inside it, (x - c)^2 or -(x - c)^2, and rescales to [0, 1]: about half the steps of trace-correcting SP2.
// Pass 0 maps the Fock matrix, X_0 = coef[1] F + coef[2] I; pass k = 1..nit applies X_k = a X_{k-1}^2 + b X_{k-1} + c I
// (coef[3k..3k+2]); every pass leaves the partial traces of X_k and X_k^2 (validation by the caller: tr(X - X^2), tr X).
// d_F is only read; d_A, d_B: two buffers of (at least) n^2 doubles; *d_res = the one holding out_scale * X_nit.
extern "C" int mi_sp2_iterate_planned(mi_ctx *c, const double *d_F, double *d_A, double *d_B, int nit, const double *coef, double out_scale,
                                      double *d_tr, double **d_tr_out, double **d_res, void *stream)
{
    if (!c || !d_F || !d_A || !d_B || !coef || !d_tr || !d_tr_out || !d_res || nit < 0) return fail("mi_sp2_iterate_planned: bad argument");
    const int n = c->nao;
    if (n > 512) return fail("mi_sp2_iterate_planned: fused path is for N <= 512");
    hipStream_t st = (hipStream_t)stream;
    const int kpad = ((n + 15) / 16) * 16;
    const size_t shm = sizeof(double) * (2 * 16 * (kpad + SP2_PAD) + 4 * 256);
    const int nb = (n + 15) / 16;
    dim3 grid(nb * (nb + 1) / 2), block(256);
    const size_t nn = (size_t)n * n;
    constexpr int TS = 2 * SP2_TRS;
    const sp2_plan_fn kern = sp2_plan_for(kpad);
    const double osc = out_scale != 0.0 ? out_scale : 1.0;
    auto next_coef = [&](int k) {   // polynomial applied in the epilogue of pass k: X_{k+1}, or the (scaled) result after the last pass
        return k < nit ? Sp2Coef{coef[3 * (k + 1)], coef[3 * (k + 1) + 1], coef[3 * (k + 1) + 2], 0.0} : Sp2Coef{0.0, osc, 0.0, 0.0};
    };
    double *cur = d_A, *nxt = d_B;
    if (c->opt_sp2_direct && kpad / 16 <= SP2_DIRECT_MAXS) {
        const int S = kpad / 16;   // MFMA steps per wave (K-quarter kpad / 4)
        const sp2_direct_fn dk = sp2_direct_for(S);
        hipLaunchKernelGGL(dk, grid, block, 0, st, d_F, n, S, coef[1], coef[2], cur, d_tr, next_coef(0));
        for (int it = 1; it <= nit; it++) {
            hipLaunchKernelGGL(dk, grid, block, 0, st, cur, n, S, 1.0, 0.0, nxt, d_tr + TS * it, next_coef(it));
            std::swap(cur, nxt);
        }
        HIPCHK(hipGetLastError());
        *d_tr_out = d_tr + TS * nit;
        *d_res = cur;
        return 0;
    }
    hipLaunchKernelGGL(kern, grid, block, shm, st, d_F, n, kpad, coef[1], coef[2], cur, d_tr, next_coef(0));
    for (int it = 1; it <= nit; it++) {
        hipLaunchKernelGGL(kern, grid, block, shm, st, cur, n, kpad, 1.0, 0.0, nxt, d_tr + TS * it, next_coef(it));
        std::swap(cur, nxt);
    }
    HIPCHK(hipGetLastError());
    *d_tr_out = d_tr + TS * nit;
    *d_res = cur;
    return 0;
}

// =================================================================================================
// Fused elementwise pieces of the SCF cycle (fewer launches per cycle)
// =================================================================================================
// F = h + J - (kscale) K (+ Vxc), and part[block] = this block's share of sum D*(h + 0.5*(J - kscale K))  [one-electron +
// Coulomb/exchange energy].  Partial sums in a FIXED order instead of atomics: the replicated algebra of a sharded run must
// give bit-identical results on every rank (the caller adds the ceil(nn/256) partials in index order).
__global__ __launch_bounds__(256) void fock_energy_kernel(const double *h, const double *J, const double *K, const double *Vxc,
                                                          const double *D, double kscale, size_t nn, double *F, double *part)
{
    __shared__ double sh[4];
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    double e = 0.0;
    if (idx < nn) {
        double v2 = J[idx] - (K ? kscale * K[idx] : 0.0);
        double f = h[idx] + v2 + (Vxc ? Vxc[idx] : 0.0);
        F[idx] = f;
        e = D[idx] * (h[idx] + 0.5 * v2);
    }
    for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = e;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

extern "C" int mi_reduce_blocks(const mi_ctx *c) { return c ? (int)(((size_t)c->nao * c->nao + 255) / 256) : -1; }

extern "C" int mi_fock_energy(mi_ctx *c, const double *d_h, const double *d_J, const double *d_K, const double *d_Vxc,
                              const double *d_D, double kscale, double *d_F, double *d_part, void *stream)
{
    if (!c || !d_h || !d_J || !d_D || !d_F || !d_part) return fail("mi_fock_energy: null argument");
    size_t nn = (size_t)c->nao * c->nao;
    hipLaunchKernelGGL(fock_energy_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_h, d_J, d_K, d_Vxc,
                       d_D, kscale, nn, d_F, d_part);
    HIPCHK(hipGetLastError());
    return 0;
}

// J/K digestion and Fock / energy assembly without the intermediate J and K matrices (single rank, resident tiles): the
// epilogue reads the padded accumulators directly,
//   J = 2 (Jacc + Jacc^T), K = Kacc + Kacc^T, F = h + J - kscale K (+ V + V^T for an UNsymmetrised XC matrix V),
//   part[block] = this block's share of sum D (h + 0.5 (J - kscale K))      (same fixed-order partials as fock_energy_kernel)
// -- one launch instead of finalize_jk_kernel + (V + V^T) + fock_energy_kernel, and 2 N^2 doubles less written and re-read.
__global__ __launch_bounds__(256) void finalize_fock_kernel(const double *Jacc, const double *Kacc, int ld, const double *h,
                                                            const double *Vun, const double *D, double kscale, int nao, double *F,
                                                            double *part, const int *__restrict__ perm)
{
    __shared__ double sh[4];
    const size_t nn = (size_t)nao * nao, idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    double e = 0.0;
    if (idx < nn) {
        const int r = (int)(idx / nao), c = (int)(idx - (size_t)r * nao);
        const int pr = perm[r], pc = perm[c];     // the accumulators are in the tile order of the ERI store
        const double j = 2.0 * (Jacc[(size_t)pr * ld + pc] + Jacc[(size_t)pc * ld + pr]);
        const double k = Kacc ? Kacc[(size_t)pr * ld + pc] + Kacc[(size_t)pc * ld + pr] : 0.0;
        const double v2 = j - (Kacc ? kscale * k : 0.0);
        const double hh = h[idx];
        F[idx] = hh + v2 + (Vun ? Vun[idx] + Vun[(size_t)c * nao + r] : 0.0);
        e = D[idx] * (hh + 0.5 * v2);
    }
    for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = e;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

extern "C" int mi_build_fock(mi_ctx *c, const double *d_D, const double *d_h, const double *d_Vun, int with_k, double kscale, double *d_F,
                             double *d_part, void *stream)
{
    if (!c || !d_D || !d_h || !d_F || !d_part) return fail("mi_build_fock: null argument");
    if (!c->eri_ready) return fail("mi_build_fock: call mi_eri_prepare first");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t nn = (size_t)c->nao * c->nao, pp = (size_t)c->ldp * c->ldp;
    hipLaunchKernelGGL(pad_density_clear_kernel, dim3((unsigned)((pp + 255) / 256)), dim3(256), 0, st, d_D, c->d_Dpad, c->d_Jacc,
                       with_k ? c->d_Kacc : nullptr, c->nao, c->ldp, c->d_iperm);
    if (launch_jk(c, true, with_k != 0, st)) return -1;
    hipLaunchKernelGGL(finalize_fock_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, st, c->d_Jacc, with_k ? c->d_Kacc : nullptr,
                       c->ldp, d_h, d_Vun, d_D, kscale, c->nao, d_F, d_part, c->d_perm);
    HIPCHK(hipGetLastError());
    return 0;
}

// E = M - M^T and part[block] = this block's share of sum E^2 (fixed-order partials, see fock_energy_kernel)
__global__ __launch_bounds__(256) void commutator_norm_kernel(const double *M, int n, double *E, double *part)
{
    __shared__ double sh[4];
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    double s = 0.0;
    if (idx < (size_t)n * n) {
        int r = (int)(idx / n), cidx = (int)(idx - (size_t)r * n);
        double v = M[idx] - M[(size_t)cidx * n + r];
        E[idx] = v;
        s = v * v;
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

extern "C" int mi_commutator_norm(mi_ctx *c, const double *d_M, double *d_E, double *d_part, void *stream)
{
    if (!c || !d_M || !d_E || !d_part) return fail("mi_commutator_norm: null argument");
    int n = c->nao;
    hipLaunchKernelGGL(commutator_norm_kernel, dim3((unsigned)(((size_t)n * n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_M, n, d_E,
                       d_part);
    HIPCHK(hipGetLastError());
    return 0;
}

// =================================================================================================
// Vxc accumulation  C[m][n] += sum_g A[m][g] * W[n][g]   (A = ao0, W = weighted AOs; K = grid dimension).
// rocBLAS runs this shape (tiny M,N ~ N_ao, K ~ 3e4) at < 1 TFLOP/s (no split-K: a handful of workgroups),
// so it is done here: 64x64 output tile per workgroup, grid.z splits the grid points, row panels staged in
// LDS (the contraction index is the contiguous one: coalesced loads), v_mfma_f64_16x16x4_f64, 2x2 MFMA tiles
// per wave, FP64 atomics to combine the splits.
// =================================================================================================
#define VM_T 64
#define VM_KS 64
#define VM_PAD 2 /* see SP2_PAD: conflict-free operand reads for 16 rows x 4 k */
__global__ __launch_bounds__(256) void xc_vmat_kernel(const double *__restrict__ A, const double *__restrict__ W, int nao, int64_t ng,
                                                      int64_t kchunk, double *C, int xcd_order)
{
    __shared__ double Pa[VM_T][VM_KS + VM_PAD], Pb[VM_T][VM_KS + VM_PAD];
    // 1-D grid of nt^2 x nsplit workgroups.  The dispatcher deals consecutive workgroups round-robin to the 8 XCDs, each with an L2
    // of its own; with the natural order the nt tiles that share a row panel of one split land on different XCDs and every XCD
    // fetches that panel itself (nt = 5: 2.6 GB through the fabric per pass at N = 264).  XCD-aware order (nsplit a multiple of 8):
    // workgroup L belongs to XCD L % 8 and works on split (L % 8) + 8 (L / (8 nt^2)), tile (L / 8) % nt^2 -- all tiles of a split
    // run next to each other on one XCD and share its L2.
    const int nt = (nao + VM_T - 1) / VM_T, ntt = nt * nt;
    const int L = (int)blockIdx.x;
    int tile, split;
    if (xcd_order) { split = (L & 7) + 8 * (L / (8 * ntt)); tile = (L >> 3) % ntt; }
    else { tile = L % ntt; split = L / ntt; }
    const int m0 = (tile / nt) * VM_T, n0 = (tile % nt) * VM_T;
    const int64_t kbeg = (int64_t)split * kchunk, kend = min(ng, kbeg + kchunk);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int qm = (wave >> 1) * 32, qn = (wave & 1) * 32;
    // which of this wave's 2 x 2 blocks of 16 rows / columns lie inside the matrix (wave-uniform)
    const bool va0 = m0 + qm < nao, va1 = m0 + qm + 16 < nao, vb0 = n0 + qn < nao, vb1 = n0 + qn + 16 < nao;
    d4_t acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) acc[a][b] = d4_t{0.0, 0.0, 0.0, 0.0};
    // register-staged software pipeline: the global loads of sub-chunk c+1 are in flight while sub-chunk c is
    // multiplied out of LDS
    constexpr int PER = VM_T * VM_KS / 256; // 16 elements of each panel per thread
    double ra[PER], rb[PER];
    auto gload = [&](int64_t k0) {
#pragma unroll
        for (int u = 0; u < PER; u++) {
            int idx = u * 256 + threadIdx.x;
            int r = idx / VM_KS, k = idx - r * VM_KS;
            int64_t g = k0 + k;
            ra[u] = (m0 + r < nao && g < kend) ? A[(size_t)(m0 + r) * ng + g] : 0.0;
            rb[u] = (n0 + r < nao && g < kend) ? W[(size_t)(n0 + r) * ng + g] : 0.0;
        }
    };
    if (kbeg < kend) gload(kbeg);
    for (int64_t k0 = kbeg; k0 < kend; k0 += VM_KS) {
#pragma unroll
        for (int u = 0; u < PER; u++) {
            int idx = u * 256 + threadIdx.x;
            int r = idx / VM_KS, k = idx - r * VM_KS;
            Pa[r][k] = ra[u];
            Pb[r][k] = rb[u];
        }
        __syncthreads();
        if (k0 + VM_KS < kend) gload(k0 + VM_KS);
        if (va1 && vb1) {
#pragma unroll 4
            for (int kk = 0; kk < VM_KS; kk += 4) {
                const int kc = kk + (lane >> 4);
                double a0 = Pa[qm + (lane & 15)][kc], a1 = Pa[qm + 16 + (lane & 15)][kc];
                double b0 = Pb[qn + (lane & 15)][kc], b1 = Pb[qn + 16 + (lane & 15)][kc];
                acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
            }
        } else if (va0 && vb0) {
            // edge tile (nao is not a multiple of 64): only the 16x16 blocks that reach into the matrix are multiplied, so the
            // mostly empty last tile row / column costs a half or a quarter of a full tile instead of the same
#pragma unroll 4
            for (int kk = 0; kk < VM_KS; kk += 4) {
                const int kc = kk + (lane >> 4);
                const double a0 = Pa[qm + (lane & 15)][kc], b0 = Pb[qn + (lane & 15)][kc];
                acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
                if (vb1) acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, Pb[qn + 16 + (lane & 15)][kc], acc[0][1], 0, 0, 0);
                if (va1) acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(Pa[qm + 16 + (lane & 15)][kc], b0, acc[1][0], 0, 0, 0);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                int row = m0 + qm + a * 16 + (lane >> 4) + 4 * r, col = n0 + qn + b * 16 + (lane & 15); // f64 MFMA C/D layout
                if (row < nao && col < nao) atomicAdd(&C[(size_t)row * nao + col], acc[a][b][r]);
            }
}

extern "C" int mi_xc_vmat(mi_ctx *c, const double *d_ao0, const double *d_aow, int64_t ng, double *d_vmat, void *stream)
{
    if (!c) return fail("mi_xc_vmat: null context");
    if (ng < 0) return fail("mi_xc_vmat: negative number of grid points");
    if (ng == 0) return 0;   // C += A W^T over no points; the split arithmetic below would divide by a zero chunk
    if (!d_ao0 || !d_aow || !d_vmat) return fail("mi_xc_vmat: null argument");
    const int nt = (c->nao + VM_T - 1) / VM_T;
    // Split over the grid points: nt^2 x nsplit workgroups, two of which fit a CU (68 KB of LDS each), i.e. 512 run at a time.
    // Round 1 rounded nsplit UP to reach 1024 -- 1025 workgroups for benzene/cc-pVTZ, 1053 for ibuprofen/def2-TZVP: a third,
    // almost empty round.  Rounding DOWN (<= 1024: two full rounds): 0.563 -> 0.525 ms (123 k points, N = 264) and 0.900 ->
    // 0.778 ms (55 k points, N = 573; 46.7 TFLOP/s = 59 % of the FP64-MFMA peak); 768 / 1536 are worse, 2048 equal, 4096 better
    // for N = 264 (0.485) and worse for N = 573 (0.836: 130 MB of split atomics) -- tools/vmat_ab.py.  Other tile shapes
    // (64x64 / 128x64 / 64x128 / 128x128 outputs, 16-64 points per LDS stage) were within +-10 % of this kernel, none better on both.
    const int64_t wgs = c->opt_vmat_wgs > 0 ? c->opt_vmat_wgs : 1024;
    int64_t nsplit = c->opt_vmat_wgs >= 0 ? std::max<int64_t>(1, std::min<int64_t>((ng + 511) / 512, wgs / (nt * nt)))
                                          : std::max<int64_t>(1, std::min<int64_t>((ng + 511) / 512, (1024 + nt * nt - 1) / (nt * nt)));
    int64_t kchunk = ((ng + nsplit - 1) / nsplit + VM_KS - 1) / VM_KS * VM_KS;
    nsplit = (ng + kchunk - 1) / kchunk;
    int xcd_order = 0;
    const int64_t ns8 = nsplit / 8 * 8;       // the XCD-aware order needs a multiple of 8 splits: taken when that costs < 10 % of them
    if (c->opt_vmat_xcd && ns8 >= 8 && ns8 * 10 >= nsplit * 9) {
        nsplit = ns8;
        kchunk = ((ng + nsplit - 1) / nsplit + VM_KS - 1) / VM_KS * VM_KS;
        xcd_order = 1;
    }
    hipLaunchKernelGGL(xc_vmat_kernel, dim3((unsigned)(nt * nt * nsplit)), dim3(256), 0, (hipStream_t)stream, d_ao0, d_aow, c->nao, ng, kchunk,
                       d_vmat, xcd_order);
    HIPCHK(hipGetLastError());
    return 0;
}

// =================================================================================================
// Vxc accumulation with the weighted AOs formed ON THE FLY (round 3):  C[m][n] += sum_g ao_0[m][g] * W[n][g],
//   W[n][g] = sum_c wv_c[g] ao_c[n][g]   (c = 0 for LDA, 0..3 for GGA)  -- what xc_aow_kernel used to write out and xc_vmat_kernel
// to read back (a 1.3 GB pass of 0.24 ms per build on benzene/cc-pVTZ that existed only to feed this product).
// Tiling: a workgroup owns MT x 64 rows (up to ALL rows of the matrix) x 64 columns and a slice of the grid points, so the
// four AO components of the B operand are read ONCE per row block instead of once per 64-row tile, and a wave holds MT x 4
// MFMA tiles (16 MT rows x 64 columns): MT + 4 LDS operand reads feed 4 MT v_mfma_f64_16x16x4_f64 per k step (0.45 reads per
// MFMA at MT = 5 against 1.0 in xc_vmat_kernel, whose counters show 52 % issue stalls at 42 % of the MFMA peak).
// =================================================================================================
#define VF_KS 16
#define VF_PAD 2
#define VF_THREADS 256
// 256 threads = 4 waves, wave w owns the 16 MT rows of slab w and all 64 columns (MT x 4 MFMA tiles), 16-point chunks.
// MEASURED SLOWER than the xc_aow + xc_vmat pair it was meant to replace (benzene/cc-pVTZ, 123 k points; the pair: 0.24 + 0.51 ms):
//   this kernel, MT = 1 / 2 / 3 (two waves per SIMD)                         1.78 / 1.26 / 1.15 ms
//   MT = 5 (all 264 rows in one workgroup, 336 VGPRs, one wave per SIMD)        1.45 ms with 32-point chunks; forced to 256 VGPRs: 2.2 ms
//   MT = 5, 512 threads, double-buffered LDS stage, one workgroup per CU      0.88 ms (32.5 % of the MFMA peak by the MOPS counter)
// The four-component B operand costs 4 loads + 3 FMAs per element in the loader of a kernel whose limit is already the
// load -> LDS -> MFMA hand-over (xc_vmat_kernel: 52 % issue stalls), and the row blocks that would amortise it do not fit the
// registers of two waves per SIMD.  Kept as an option (`RKS.xc_vmat_fold`, default off), not used.
template <int MT>
__global__ __launch_bounds__(VF_THREADS) void xc_vmat_fold_kernel(const double *__restrict__ ao, const double *__restrict__ wv, int ncomp, int nao,
                                                                  int64_t ng, int64_t kchunk, int nct, int nrb, double *C, int xcd_order)
{
    extern __shared__ double lds_all[];
    constexpr int MR = MT * 64, LDS_LD = VF_KS + VF_PAD;
    double *Pa = lds_all, *Pb = lds_all + (size_t)MR * LDS_LD;
    const int ntt = nct * nrb;
    const int L = (int)blockIdx.x;
    int tile, split;
    if (xcd_order) { split = (L & 7) + 8 * (L / (8 * ntt)); tile = (L >> 3) % ntt; }
    else { tile = L % ntt; split = L / ntt; }
    const int rb = tile / nct, ct = tile - rb * nct;
    const int m0 = rb * MR, n0 = ct * 64;
    const int64_t kbeg = (int64_t)split * kchunk, kend = min(ng, kbeg + kchunk);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wr0 = wave * (MT * 16);
    const size_t comp = (size_t)nao * ng;
    d4_t acc[MT][4];
#pragma unroll
    for (int a = 0; a < MT; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) acc[a][b] = d4_t{0.0, 0.0, 0.0, 0.0};
    constexpr int PA = MR * VF_KS / VF_THREADS, PB = 64 * VF_KS / VF_THREADS;   // 4 MT and 4 elements per thread
    const int kq = threadIdx.x & (VF_KS - 1), rq = threadIdx.x >> 4;           // element u of a thread: row rq + 16 u, point kq
    double ra[PA], rb_[PB];
    auto gload = [&](int64_t k0) {
        const int64_t g = k0 + kq;
        const bool gv = g < kend;
        double w0 = 0.0, w1 = 0.0, w2 = 0.0, w3 = 0.0;
        if (gv) {
            w0 = wv[g];
            if (ncomp > 1) { w1 = wv[ng + g]; w2 = wv[2 * ng + g]; w3 = wv[3 * ng + g]; }
        }
        const double *pa = ao + (size_t)(m0 + rq) * ng + g;
#pragma unroll
        for (int u = 0; u < PA; u++) ra[u] = (gv && m0 + rq + 16 * u < nao) ? pa[(size_t)(16 * u) * ng] : 0.0;
        const double *pb = ao + (size_t)(n0 + rq) * ng + g;
#pragma unroll
        for (int u = 0; u < PB; u++) {
            double v = 0.0;
            if (gv && n0 + rq + 16 * u < nao) {
                const double *q = pb + (size_t)(16 * u) * ng;
                v = q[0] * w0;
                if (ncomp > 1) v = fma(q[comp], w1, fma(q[2 * comp], w2, fma(q[3 * comp], w3, v)));
            }
            rb_[u] = v;
        }
    };
    if (kbeg < kend) gload(kbeg);
    const bool rows_in = m0 + wr0 < nao;   // wave-uniform
    for (int64_t k0 = kbeg; k0 < kend; k0 += VF_KS) {
#pragma unroll
        for (int u = 0; u < PA; u++) Pa[(rq + 16 * u) * LDS_LD + kq] = ra[u];
#pragma unroll
        for (int u = 0; u < PB; u++) Pb[(rq + 16 * u) * LDS_LD + kq] = rb_[u];
        __syncthreads();
        if (k0 + VF_KS < kend) gload(k0 + VF_KS);       // in flight while this chunk is multiplied
        if (rows_in) {
#pragma unroll
            for (int kk = 0; kk < VF_KS; kk += 4) {
                const int kc = kk + (lane >> 4);
                double b[4];
#pragma unroll
                for (int j = 0; j < 4; j++) b[j] = Pb[(j * 16 + (lane & 15)) * LDS_LD + kc];
#pragma unroll
                for (int a = 0; a < MT; a++) {
                    const double av = Pa[(wr0 + a * 16 + (lane & 15)) * LDS_LD + kc];
#pragma unroll
                    for (int j = 0; j < 4; j++) acc[a][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b[j], acc[a][j], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < MT; a++)
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int row = m0 + wr0 + a * 16 + (lane >> 4) + 4 * r, col = n0 + j * 16 + (lane & 15);   // f64 MFMA C/D layout
                if (row < nao && col < nao) atomicAdd(&C[(size_t)row * nao + col], acc[a][j][r]);
            }
}

template <int MT>
static int launch_vmat_fold(mi_ctx *c, const double *d_ao, const double *d_wv, int ncomp, int64_t ng, int nrb, double *d_vmat, hipStream_t st)
{
    const int nct = (c->nao + 63) / 64, ntt = nct * nrb;
    const size_t shm = sizeof(double) * (size_t)(MT * 64 + 64) * (VF_KS + VF_PAD);
    // one workgroup per CU fits (LDS) at MT = 5: aim at one full round of workgroups, at least 512 points per split
    const int64_t wgs = c->opt_vmat_wgs > 0 ? c->opt_vmat_wgs : 512;   // two workgroups per CU
    int64_t nsplit = std::max<int64_t>(1, std::min<int64_t>((ng + 511) / 512, wgs / ntt));
    int64_t kchunk = ((ng + nsplit - 1) / nsplit + VF_KS - 1) / VF_KS * VF_KS;
    nsplit = (ng + kchunk - 1) / kchunk;
    int xcd_order = 0;
    const int64_t ns8 = nsplit / 8 * 8;
    if (c->opt_vmat_xcd && ns8 >= 8 && ns8 * 10 >= nsplit * 9) {
        nsplit = ns8;
        kchunk = ((ng + nsplit - 1) / nsplit + VF_KS - 1) / VF_KS * VF_KS;
        xcd_order = 1;
    }
    if (shm > 64 * 1024) HIPCHK(hipFuncSetAttribute((const void *)xc_vmat_fold_kernel<MT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
    hipLaunchKernelGGL((xc_vmat_fold_kernel<MT>), dim3((unsigned)(ntt * nsplit)), dim3(VF_THREADS), shm, st, d_ao, d_wv, ncomp, c->nao, ng, kchunk, nct, nrb,
                       d_vmat, xcd_order);
    HIPCHK(hipGetLastError());
    return 0;
}

// d_ao: [ncomp >= 1 | 4][nao][ng] AO values (component 0 = values, 1..3 = gradient), d_wv: [1 | 4][ng] weights x potential
// (as mi_xc_aow takes them), gga = 0: LDA (component 0 only).  d_vmat += ao_0 . (sum_c wv_c ao_c)^T, unsymmetrised.
extern "C" int mi_xc_vmat_fold(mi_ctx *c, const double *d_ao, const double *d_wv, int64_t ng, int gga, double *d_vmat, void *stream)
{
    if (!c) return fail("mi_xc_vmat_fold: null context");
    if (ng < 0) return fail("mi_xc_vmat_fold: negative number of grid points");
    if (ng == 0) return 0;   // as mi_xc_vmat: no points, no launch
    if (!d_ao || !d_wv || !d_vmat) return fail("mi_xc_vmat_fold: null argument");
    hipStream_t st = (hipStream_t)stream;
    const int nt = (c->nao + 63) / 64;                 // 64-row tiles of the matrix
    const int cap = std::max(1, std::min(5, c->opt_vmat_fold_mt));
    const int nrb = (nt + cap - 1) / cap;              // row blocks of at most `cap` 64-row tiles (registers: two waves per SIMD up to 3)
    const int mt = (nt + nrb - 1) / nrb;               // tiles per row block
    const int ncomp = gga ? 4 : 1;
    switch (mt) {
    case 1: return launch_vmat_fold<1>(c, d_ao, d_wv, ncomp, ng, nrb, d_vmat, st);
    case 2: return launch_vmat_fold<2>(c, d_ao, d_wv, ncomp, ng, nrb, d_vmat, st);
    case 3: return launch_vmat_fold<3>(c, d_ao, d_wv, ncomp, ng, nrb, d_vmat, st);
    case 4: return launch_vmat_fold<4>(c, d_ao, d_wv, ncomp, ng, nrb, d_vmat, st);
    default: return launch_vmat_fold<5>(c, d_ao, d_wv, ncomp, ng, nrb, d_vmat, st);
    }
}

// =================================================================================================
// C-PCM implicit solvation (mi355scf/pcm.py): one-electron integrals against the Gaussian surface charges of the cavity.
//
//   B[g, mn] = int phi_m phi_n erf(zeta_g |r - s_g|) / |r - s_g| dr,   rows g = surface points, columns mn = packed spherical
//   AO pairs m >= n (caller's AO order, column m (m + 1) / 2 + n), row stride ld >= nao (nao + 1) / 2 (padding columns zero).
//
// The attenuated nuclear attraction by Rys quadrature: with eta = zeta^2 and rho = p eta / (p + eta) the Boys argument is
// rho |PC|^2, the prefactor gains sqrt(rho / p) and the roots are scaled by rho / p before the usual 1-D recurrences.
// Every launch holds shell pairs of ONE angular class (template arguments: fixed-size register arrays, no per-thread blocks
// sized for the largest class); a workgroup is (one shell pair, up to 64 surface points of one owning atom).
//   pcm_int_kernel<LA,LB>       B (once per geometry)
//   pcm_potential_kernel        v[g] = vn[g] - sum_c B[g,c] d[c]     (per cycle; one workgroup per row, fixed-order sums)
//   pcm_fock_partial_kernel     part[k][c] = sum_{g in chunk k} q[g] B[g,c]   (per cycle; column-streaming, no atomics)
//   pcm_fock_finalize_kernel    V[m,n] (+)= scale sum_k part[k][c(m,n)]        (chunks added in index order)
//   pcm_grad_kernel<LA,LB>      -2 sum_g q_g sum_{m in A, n} D_mn <d_A m|erf/r|n> per (ordered pair, point block)
// =================================================================================================
struct PcmArgs : BasisDev {
    const int *pairs;     // [n][2] shell pairs of one class (la, lb) = template arguments
    const double *pts;    // [npts][4]: x, y, z, zeta
    const int *blk;       // [nblk][3]: first point, count (1..64), owning atom
    int nblk;
    int64_t ld;
    double *B;
    const double *D, *q;  // gradient: density [nao][nao], surface charges [npts]
    double *part;         // gradient: [n][nblk][3] (rows of the launch's class at its offset)
};

template <int LA, int LB>
__global__ __launch_bounds__(64) void pcm_int_kernel(PcmArgs A)
{
    constexpr int NCA = (LA + 1) * (LA + 2) / 2, NCB = (LB + 1) * (LB + 2) / 2, NSA = 2 * LA + 1, NSB = 2 * LB + 1;
    constexpr int NR = (LA + LB) / 2 + 1, NI = LA + LB + 1;
    const int pidx = blockIdx.x / A.nblk, b = blockIdx.x - pidx * A.nblk;
    const int *bk = A.blk + 3 * b;
    if ((int)threadIdx.x >= bk[1]) return;
    const int g = bk[0] + threadIdx.x;
    const int ish = A.pairs[2 * pidx], jsh = A.pairs[2 * pidx + 1];
    const int32_t *bi = A.bas + ish * BAS_SLOTS, *bj = A.bas + jsh * BAS_SLOTS;
    const double *ra = A.env + A.atm[bi[0] * ATM_SLOTS + 1], *rb = A.env + A.atm[bj[0] * ATM_SLOTS + 1];
    const double C[3] = {A.pts[4 * g], A.pts[4 * g + 1], A.pts[4 * g + 2]};
    const double eta = A.pts[4 * g + 3] * A.pts[4 * g + 3];
    const double AB[3] = {ra[0] - rb[0], ra[1] - rb[1], ra[2] - rb[2]};
    double acc[NCA * NCB];
#pragma unroll
    for (int k = 0; k < NCA * NCB; k++) acc[k] = 0.0;
    for (int ip = 0; ip < bi[2]; ip++)
        for (int jp = 0; jp < bj[2]; jp++) {
            const PrimPair q = prim_pair(A.env, bi, bj, ip, jp, ra, rb, AB);
#pragma unroll
            for (int r = 0; r < NR; r++) {
                double gt[3][NI][LB + 1];
                const double f = attraction_table<LB, NI, true>(gt, q, C, eta, AB, NR, r, A.rys);
                attraction_accumulate<LA, LB>(acc, gt, f);
            }
        }
    const double *ca = A.c2s + A.c2s_off[LA], *cb = A.c2s + A.c2s_off[LB];
    const int ao_i = A.shell_ao[ish], ao_j = A.shell_ao[jsh];
    double *row = A.B + (size_t)g * A.ld;
    for (int i = 0; i < NSA; i++)
        for (int j = 0; j < NSB; j++) {
            int m = ao_i + i, n = ao_j + j;
            if (ish == jsh && n > m) continue;
            const double v = block_to_spherical<LA, LB>(acc, ca, cb, i, j);
            if (m < n) { const int s_ = m; m = n; n = s_; }
            row[(size_t)m * (m + 1) / 2 + n] = v;
        }
}

template <int LA, int LB>
__global__ __launch_bounds__(64) void pcm_grad_kernel(PcmArgs A)
{
    constexpr int NCA = (LA + 1) * (LA + 2) / 2, NCB = (LB + 1) * (LB + 2) / 2;
    constexpr int NR = (LA + LB + 1) / 2 + 1, NI = LA + LB + 2;
    __shared__ double Dc[NCA * NCB];
    const int pidx = blockIdx.x / A.nblk, b = blockIdx.x - pidx * A.nblk;
    const int *bk = A.blk + 3 * b;
    const int ish = A.pairs[2 * pidx], jsh = A.pairs[2 * pidx + 1];
    const int32_t *bi = A.bas + ish * BAS_SLOTS, *bj = A.bas + jsh * BAS_SLOTS;
    const int ao_i = A.shell_ao[ish], ao_j = A.shell_ao[jsh];
    const double *ca = A.c2s + A.c2s_off[LA], *cb = A.c2s + A.c2s_off[LB];
    for (int k = threadIdx.x; k < NCA * NCB; k += 64)   // density block back-transformed to cartesian components, once per workgroup
        Dc[k] = density_block_to_cartesian<LA, LB>(A.D, A.nao, ao_i, ao_j, ca, cb, k / NCB, k % NCB);
    __syncthreads();
    double gc[3] = {0.0, 0.0, 0.0};
    if ((int)threadIdx.x < bk[1]) {
        const int g = bk[0] + threadIdx.x;
        const double *ra = A.env + A.atm[bi[0] * ATM_SLOTS + 1], *rb = A.env + A.atm[bj[0] * ATM_SLOTS + 1];
        const double C[3] = {A.pts[4 * g], A.pts[4 * g + 1], A.pts[4 * g + 2]};
        const double eta = A.pts[4 * g + 3] * A.pts[4 * g + 3];
        const double qg = A.q[g];
        const double AB[3] = {ra[0] - rb[0], ra[1] - rb[1], ra[2] - rb[2]};
        for (int ip = 0; ip < bi[2]; ip++)
            for (int jp = 0; jp < bj[2]; jp++) {
                PrimPair q = prim_pair(A.env, bi, bj, ip, jp, ra, rb, AB);
                q.cc = qg * q.cc;   // the point's charge rides on the prefactor
#pragma unroll
                for (int r = 0; r < NR; r++) {
                    double gt[3][NI][LB + 1];
                    const double f = attraction_table<LB, NI, true>(gt, q, C, eta, AB, NR, r, A.rys);
                    attraction_bra_gradient<LA, LB>(gc, gt, f, q.a, Dc);
                }
            }
    }
    // butterfly over the wave: every lane ends with the same fixed-order sum (no atomics)
#pragma unroll
    for (int d = 0; d < 3; d++)
        for (int o = 32; o > 0; o >>= 1) gc[d] += __shfl_xor(gc[d], o);
    if (threadIdx.x == 0)
        for (int d = 0; d < 3; d++) A.part[((size_t)pidx * A.nblk + b) * 3 + d] = -2.0 * gc[d];
}

__global__ __launch_bounds__(256) void pcm_pack_kernel(const double *D, int nao, double *d)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)nao * nao) return;
    const int m = (int)(idx / nao), n = (int)(idx - (size_t)m * nao);
    if (n > m) return;
    d[(size_t)m * (m + 1) / 2 + n] = m == n ? D[idx] : D[idx] + D[(size_t)n * nao + m];
}

__global__ __launch_bounds__(256) void pcm_potential_kernel(const double *B, int64_t ld, const double *d, const double *vn, double *v)
{
    __shared__ double sh[4];
    const int64_t g = blockIdx.x;
    const d2_t *row = reinterpret_cast<const d2_t *>(B + g * ld);
    const d2_t *d2 = reinterpret_cast<const d2_t *>(d);
    const int64_t n2 = ld / 2;
    double s0 = 0.0, s1 = 0.0;
    int64_t c = threadIdx.x;
    for (; c + 256 < n2; c += 512) {
        const d2_t b0 = __builtin_nontemporal_load(row + c), b1 = __builtin_nontemporal_load(row + c + 256);
        const d2_t e0 = d2[c], e1 = d2[c + 256];
        s0 += b0.x * e0.x + b0.y * e0.y;
        s1 += b1.x * e1.x + b1.y * e1.y;
    }
    if (c < n2) {
        const d2_t b0 = __builtin_nontemporal_load(row + c), e0 = d2[c];
        s0 += b0.x * e0.x + b0.y * e0.y;
    }
    double s = s0 + s1;
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double t = (sh[0] + sh[1]) + (sh[2] + sh[3]);
        v[g] = vn ? vn[g] - t : t;
    }
}

__global__ __launch_bounds__(256) void pcm_fock_partial_kernel(const double *B, int64_t ld, int npts, int rows_per, const double *q, double *part)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= ld / 2) return;
    const int g0 = blockIdx.y * rows_per, g1 = min(npts, g0 + rows_per);
    double ax = 0.0, ay = 0.0, bx = 0.0, by = 0.0;
    int g = g0;
    for (; g + 1 < g1; g += 2) {
        const d2_t b0 = __builtin_nontemporal_load(reinterpret_cast<const d2_t *>(B + (int64_t)g * ld) + c);
        const d2_t b1 = __builtin_nontemporal_load(reinterpret_cast<const d2_t *>(B + (int64_t)(g + 1) * ld) + c);
        const double q0 = q[g], q1 = q[g + 1];
        ax += q0 * b0.x; ay += q0 * b0.y;
        bx += q1 * b1.x; by += q1 * b1.y;
    }
    if (g < g1) {
        const d2_t b0 = __builtin_nontemporal_load(reinterpret_cast<const d2_t *>(B + (int64_t)g * ld) + c);
        ax += q[g] * b0.x; ay += q[g] * b0.y;
    }
    d2_t out;
    out.x = ax + bx;
    out.y = ay + by;
    reinterpret_cast<d2_t *>(part + (int64_t)blockIdx.y * ld)[c] = out;
}

__global__ __launch_bounds__(256) void pcm_fock_finalize_kernel(const double *part, int nchunk, int64_t ld, int nao, double scale, int accumulate,
                                                                double *V)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)nao * nao) return;
    const int m = (int)(idx / nao), n = (int)(idx - (size_t)m * nao);
    const int64_t c = m >= n ? (int64_t)m * (m + 1) / 2 + n : (int64_t)n * (n + 1) / 2 + m;
    double s = 0.0;
    for (int k = 0; k < nchunk; k++) s += part[(int64_t)k * ld + c];
    V[idx] = (accumulate ? V[idx] : 0.0) + scale * s;
}

// rows of the context's class-sorted pair list (shell_pair_classes): the order of B's launches and of `part`'s rows
extern "C" int mi_pcm_pairs(mi_ctx *c, int ordered, int32_t *out)
{
    if (!c) return fail("mi_pcm_pairs: null context");
    const std::vector<int> &pairs = c->pair_classes[ordered ? 1 : 0].pairs;
    if (out) std::copy(pairs.begin(), pairs.end(), out);
    return (int)(pairs.size() / 2);
}

template <bool GRAD>
static int pcm_dispatch(mi_ctx *c, PcmArgs &A, hipStream_t st)
{
    return launch_pair_classes<GRAD>(c, A.nblk, "mi_pcm", [&](auto la, auto lb, int first, int count) {
        constexpr int LA = decltype(la)::value, LB = decltype(lb)::value;
        PcmArgs B = A;
        B.pairs = c->pair_classes[GRAD].d_pairs + 2 * first;
        const dim3 grid((unsigned)((int64_t)count * A.nblk));
        if constexpr (GRAD) {
            B.part = A.part + (size_t)first * A.nblk * 3;
            hipLaunchKernelGGL((pcm_grad_kernel<LA, LB>), grid, dim3(64), 0, st, B);
        } else {
            hipLaunchKernelGGL((pcm_int_kernel<LA, LB>), grid, dim3(64), 0, st, B);
        }
    });
}

static int pcm_check_points(const mi_ctx *c, const char *who, const double *d_pts, int npts, const int32_t *d_blk, int nblk)
{
    if (!c || !d_pts || !d_blk) return fail("%s: null argument", who);
    if (check_orbital_lmax(c, who)) return -1;
    if (npts <= 0 || nblk <= 0) return fail("%s: no surface points", who);
    return 0;
}

extern "C" int mi_pcm_eval(mi_ctx *c, const double *d_pts, int npts, const int32_t *d_blk, int nblk, int64_t ld, double *d_B, void *stream)
{
    if (pcm_check_points(c, "mi_pcm_eval", d_pts, npts, d_blk, nblk)) return -1;
    if (!d_B) return fail("mi_pcm_eval: null B");
    if (ld < (int64_t)c->nao * (c->nao + 1) / 2 || (ld & 1)) return fail("mi_pcm_eval: ld = %lld must be even and >= nao (nao + 1) / 2", (long long)ld);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(d_B, 0, sizeof(double) * (size_t)npts * ld, st));
    PcmArgs A{basis_dev(c)};
    A.pts = d_pts; A.blk = d_blk; A.nblk = nblk; A.ld = ld; A.B = d_B;
    return pcm_dispatch<false>(c, A, st);
}

extern "C" int mi_pcm_grad(mi_ctx *c, const double *d_pts, int npts, const int32_t *d_blk, int nblk, const double *d_D, const double *d_q,
                           double *d_part, void *stream)
{
    if (pcm_check_points(c, "mi_pcm_grad", d_pts, npts, d_blk, nblk)) return -1;
    if (!d_D || !d_q || !d_part) return fail("mi_pcm_grad: null argument");
    HIPCHK(hipSetDevice(c->device));
    PcmArgs A{basis_dev(c)};
    A.pts = d_pts; A.blk = d_blk; A.nblk = nblk; A.D = d_D; A.q = d_q; A.part = d_part;
    return pcm_dispatch<true>(c, A, (hipStream_t)stream);
}

extern "C" int mi_pcm_potential(mi_ctx *c, const double *d_B, int npts, int64_t ld, const double *d_D, double *d_dpack, const double *d_vn,
                                double *d_v, void *stream)
{
    if (!c || !d_B || !d_D || !d_dpack || !d_v) return fail("mi_pcm_potential: null argument");
    if (npts <= 0 || ld < (int64_t)c->nao * (c->nao + 1) / 2 || (ld & 1)) return fail("mi_pcm_potential: bad sizes");
    hipStream_t st = (hipStream_t)stream;
    const size_t nn = (size_t)c->nao * c->nao;
    hipLaunchKernelGGL(pcm_pack_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, st, d_D, c->nao, d_dpack);
    hipLaunchKernelGGL(pcm_potential_kernel, dim3((unsigned)npts), dim3(256), 0, st, d_B, ld, d_dpack, d_vn, d_v);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int mi_pcm_fock_chunks(int npts, int64_t ld)
{
    const int64_t colblk = (ld / 2 + 255) / 256;
    int64_t k = (2048 + colblk - 1) / colblk;
    k = std::max<int64_t>(1, std::min<int64_t>({k, 64, (int64_t)std::max(npts, 1)}));
    return (int)k;
}

extern "C" int mi_pcm_fock(mi_ctx *c, const double *d_B, int npts, int64_t ld, const double *d_q, double scale, int accumulate, double *d_part,
                           double *d_V, void *stream)
{
    if (!c || !d_B || !d_q || !d_part || !d_V) return fail("mi_pcm_fock: null argument");
    if (npts <= 0 || ld < (int64_t)c->nao * (c->nao + 1) / 2 || (ld & 1)) return fail("mi_pcm_fock: bad sizes");
    hipStream_t st = (hipStream_t)stream;
    const int nchunk = mi_pcm_fock_chunks(npts, ld);
    const int rows_per = (npts + nchunk - 1) / nchunk;
    hipLaunchKernelGGL(pcm_fock_partial_kernel, dim3((unsigned)((ld / 2 + 255) / 256), (unsigned)nchunk), dim3(256), 0, st, d_B, ld, npts, rows_per,
                       d_q, d_part);
    const size_t nn = (size_t)c->nao * c->nao;
    hipLaunchKernelGGL(pcm_fock_finalize_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, st, d_part, nchunk, ld, c->nao, scale,
                       accumulate, d_V);
    HIPCHK(hipGetLastError());
    return 0;
}

// =================================================================================================
// Point-charge embedding (mi355scf/qmmm.py): the attraction integrals of the C-PCM section against an explicit environment of
// 10^4 .. 10^5 sites, formed, contracted and discarded in one pass -- nothing of size pairs x points is ever stored.
//
//   pts[k] = (x, y, z, zeta) in Bohr: zeta <= 0 a point charge (1/r, the nuclear body), zeta > 0 a Gaussian charge
//   (erf(zeta r)/r, the PCM body); both run the attenuated table, which reproduces the plain one exactly at theta = 1 (pc_eta).
//
//   pc_fock_kernel<LA,LB>   workgroup = (shell pair i >= j, chunk of points); the lanes stride over the chunk's points with the
//                           cartesian block in registers, one butterfly per block, cart -> sph by the first NSA NSB lanes and
//                           a write into part[chunk][packed column]; pcm_fock_finalize_kernel adds the chunks in index order
//   pc_grad_kernel<LA,LB>   workgroup = (chunk of ordered pairs, block of 64 .. PC_GRAD_POINTS sites); per pair the density block goes
//                           to LDS once, each lane walks its points; the bra derivative is summed over the block's points per
//                           pair (butterfly -> apart[pair][block][3], the share of the atom of shell i) and over the chunk's
//                           pairs per point (lane-owned LDS slots -> ppart[pair chunk][point][3], the point's share is minus it)
//   pc_grad_atoms_kernel, pc_grad_points_kernel   the two partial arrays summed in fixed order (no atomics anywhere)
// =================================================================================================
#define PC_FOCK_POINTS 256   /* smallest chunk of mi_pc_fock: four points per lane */
#define PC_FOCK_CHUNKS 64    /* most chunks of mi_pc_fock: beyond PC_FOCK_POINTS * PC_FOCK_CHUNKS points the chunks grow */
#define PC_GRAD_POINTS 512   /* largest point block of mi_pc_grad: 12 KB of lane-owned LDS accumulators */

struct PcArgs : BasisDev {
    const int *pairs;      // [n][2] shell pairs of one class (la, lb) = template arguments
    const double *pts;     // [npts][4]: x, y, z, zeta
    const double *q;       // [npts]
    int npts;
    int per, nchunk;       // Fock: points per chunk, chunks
    int64_t ld;
    double *part;          // Fock: [nchunk][ld]
    const double *D;       // gradient: density [nao][nao]
    int npair, kpairs, nblk, pblk;   // gradient: pairs of the class, pairs per pair chunk, point blocks, sites per block
    double *apart;         // gradient: [pairs of the class][nblk][3] at the class' offset
    double *ppart;         // gradient: [pair chunks of the class][npts][3] at the class' offset
};

// eta of a site for attraction_table<.., true>: zeta^2, and for a point charge a value so large that theta = eta / (p + eta)
// rounds to exactly 1 for every exponent p -- the attenuated body then IS the plain one bit for bit (x 1, sqrt(1), u 1), and
// the two kinds share one instruction stream instead of a divergent branch around two copies of the recurrences
#define PC_POINT_ETA 1e300
__device__ __forceinline__ double pc_eta(double zeta) { return zeta > 0.0 ? zeta * zeta : PC_POINT_ETA; }

template <int LA, int LB>
__global__ __launch_bounds__(64) void pc_fock_kernel(PcArgs A)
{
    constexpr int NCA = (LA + 1) * (LA + 2) / 2, NCB = (LB + 1) * (LB + 2) / 2, NSA = 2 * LA + 1, NSB = 2 * LB + 1;
    constexpr int NR = (LA + LB) / 2 + 1, NI = LA + LB + 1;
    const int pidx = blockIdx.x / A.nchunk, k = blockIdx.x - pidx * A.nchunk;
    const int g0 = k * A.per, g1 = min(A.npts, g0 + A.per);
    const int ish = A.pairs[2 * pidx], jsh = A.pairs[2 * pidx + 1];
    const int32_t *bi = A.bas + ish * BAS_SLOTS, *bj = A.bas + jsh * BAS_SLOTS;
    const double *ra = A.env + A.atm[bi[0] * ATM_SLOTS + 1], *rb = A.env + A.atm[bj[0] * ATM_SLOTS + 1];
    const double AB[3] = {ra[0] - rb[0], ra[1] - rb[1], ra[2] - rb[2]};
    double acc[NCA * NCB];
#pragma unroll
    for (int e = 0; e < NCA * NCB; e++) acc[e] = 0.0;
    for (int g = g0 + (int)threadIdx.x; g < g1; g += 64) {
        const double C[3] = {A.pts[4 * g], A.pts[4 * g + 1], A.pts[4 * g + 2]};
        const double eta = pc_eta(A.pts[4 * g + 3]), qg = A.q[g];
        for (int ip = 0; ip < bi[2]; ip++)
            for (int jp = 0; jp < bj[2]; jp++) {
                PrimPair q = prim_pair(A.env, bi, bj, ip, jp, ra, rb, AB);
                q.cc = qg * q.cc;   // the point's charge rides on the prefactor
#pragma unroll
                for (int r = 0; r < NR; r++) {
                    double gt[3][NI][LB + 1];
                    const double f = attraction_table<LB, NI, true>(gt, q, C, eta, AB, NR, r, A.rys);
                    attraction_accumulate<LA, LB>(acc, gt, f);
                }
            }
    }
    // butterfly over the wave: every lane ends with the same fixed-order sum of the chunk (no atomics)
#pragma unroll
    for (int e = 0; e < NCA * NCB; e++)
        for (int o = 32; o > 0; o >>= 1) acc[e] += __shfl_xor(acc[e], o);
    if ((int)threadIdx.x >= NSA * NSB) return;
    const int i = threadIdx.x / NSB, j = threadIdx.x - i * NSB;
    int m = A.shell_ao[ish] + i, n = A.shell_ao[jsh] + j;
    if (ish == jsh && n > m) return;
    const double v = block_to_spherical<LA, LB>(acc, A.c2s + A.c2s_off[LA], A.c2s + A.c2s_off[LB], i, j);
    if (m < n) { const int s_ = m; m = n; n = s_; }
    A.part[(int64_t)k * A.ld + (int64_t)m * (m + 1) / 2 + n] = v;
}

template <int LA, int LB>
__global__ __launch_bounds__(64) void pc_grad_kernel(PcArgs A)
{
    constexpr int NCA = (LA + 1) * (LA + 2) / 2, NCB = (LB + 1) * (LB + 2) / 2;
    constexpr int NR = (LA + LB + 1) / 2 + 1, NI = LA + LB + 2;
    constexpr int ROOT_UNROLL = LA + LB >= 5 ? 1 : NR;   // the three heaviest classes keep one table alive (below)
    __shared__ double Dc[NCA * NCB];
    __shared__ double gp[3][PC_GRAD_POINTS];   // slot s belongs to lane s % 64 alone: no synchronisation, fixed order
    __shared__ double ga[3][64];               // the pair's sum over the lane's sites, kept out of the registers
    const int cidx = blockIdx.x / A.nblk, b = blockIdx.x - cidx * A.nblk;
    const int g0 = b * A.pblk, g1 = min(A.npts, g0 + A.pblk);
    const int p0 = cidx * A.kpairs, p1 = min(A.npair, p0 + A.kpairs);
    for (int s = threadIdx.x; s < A.pblk; s += 64) gp[0][s] = gp[1][s] = gp[2][s] = 0.0;
#pragma nounroll
    for (int p = p0; p < p1; p++) {
        const int ish = A.pairs[2 * p], jsh = A.pairs[2 * p + 1];
        const int32_t *bi = A.bas + ish * BAS_SLOTS, *bj = A.bas + jsh * BAS_SLOTS;
        const int ao_i = A.shell_ao[ish], ao_j = A.shell_ao[jsh];
        const double *ca = A.c2s + A.c2s_off[LA], *cb = A.c2s + A.c2s_off[LB];
        __syncthreads();   // the previous pair's block has been read by every lane
        for (int e = threadIdx.x; e < NCA * NCB; e += 64)   // density block back-transformed to cartesian components, once per pair
            Dc[e] = density_block_to_cartesian<LA, LB>(A.D, A.nao, ao_i, ao_j, ca, cb, e / NCB, e % NCB);
        __syncthreads();
        const double *ra = A.env + A.atm[bi[0] * ATM_SLOTS + 1], *rb = A.env + A.atm[bj[0] * ATM_SLOTS + 1];
        const double AB[3] = {ra[0] - rb[0], ra[1] - rb[1], ra[2] - rb[2]};
        ga[0][threadIdx.x] = ga[1][threadIdx.x] = ga[2][threadIdx.x] = 0.0;
#pragma nounroll
        for (int s = threadIdx.x; g0 + s < g1; s += 64) {
            const int g = g0 + s;
            const double C[3] = {A.pts[4 * g], A.pts[4 * g + 1], A.pts[4 * g + 2]};
            const double eta = pc_eta(A.pts[4 * g + 3]), qg = A.q[g];
            double gc[3] = {0.0, 0.0, 0.0};
            // <2,3>, <3,2>, <3,3>: no unrolling of the root loop -- unrolled, <3,3> keeps four tables alive and spills 1.9 KB per lane
#pragma nounroll
            for (int ip = 0; ip < bi[2]; ip++)
#pragma nounroll
                for (int jp = 0; jp < bj[2]; jp++) {
                    PrimPair q = prim_pair(A.env, bi, bj, ip, jp, ra, rb, AB);
                    q.cc = qg * q.cc;   // the point's charge rides on the prefactor
#pragma unroll ROOT_UNROLL
                    for (int r = 0; r < NR; r++) {
                        double gt[3][NI][LB + 1];
                        const double f = attraction_table<LB, NI, true>(gt, q, C, eta, AB, NR, r, A.rys);
                        attraction_bra_gradient<LA, LB>(gc, gt, f, q.a, Dc);
                    }
                }
#pragma unroll
            for (int d = 0; d < 3; d++) {
                ga[d][threadIdx.x] += gc[d];
                gp[d][s] += gc[d];
            }
        }
        // butterfly over the wave: a fixed-order sum of the block's sites (no atomics)
#pragma unroll
        for (int d = 0; d < 3; d++) {
            double t = ga[d][threadIdx.x];
            for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
            if (threadIdx.x == 0) A.apart[((int64_t)p * A.nblk + b) * 3 + d] = t;
        }
    }
    for (int s = threadIdx.x; g0 + s < g1; s += 64)
        for (int d = 0; d < 3; d++) A.ppart[((int64_t)cidx * A.npts + g0 + s) * 3 + d] = gp[d][s];
}

// out[a] = 2 sum over the ordered pairs whose first shell sits on atom a, over the point blocks: thread t takes pairs t, t + 256, ..
// in order, then a fixed tree over the threads
__global__ __launch_bounds__(256) void pc_grad_atoms_kernel(const double *apart, const int *pairs, const int32_t *bas, int npair, int nblk,
                                                            double *out)
{
    __shared__ double sh[3][256];
    const int a = blockIdx.x;
    double s[3] = {0.0, 0.0, 0.0};
    for (int p = threadIdx.x; p < npair; p += 256) {
        if (bas[pairs[2 * p] * BAS_SLOTS] != a) continue;
        const double *row = apart + (int64_t)p * nblk * 3;
        for (int b = 0; b < nblk; b++)
            for (int d = 0; d < 3; d++) s[d] += row[3 * b + d];
    }
    for (int d = 0; d < 3; d++) sh[d][threadIdx.x] = s[d];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o)
            for (int d = 0; d < 3; d++) sh[d][threadIdx.x] += sh[d][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x < 3) out[3 * a + threadIdx.x] = 2.0 * sh[threadIdx.x][0];
}

// out[g][d] = -2 sum_c ppart[c][g][d], pair chunks in index order
__global__ __launch_bounds__(256) void pc_grad_points_kernel(const double *ppart, int nchunk, int64_t n3, double *out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n3) return;
    double s = 0.0;
    for (int c = 0; c < nchunk; c++) s += ppart[(int64_t)c * n3 + i];
    out[i] = -2.0 * s;
}

// points per chunk of mi_pc_fock: PC_FOCK_POINTS until there would be more than PC_FOCK_CHUNKS chunks, then whole waves more
static int pc_fock_points(int npts)
{
    const int per = (npts + PC_FOCK_CHUNKS - 1) / PC_FOCK_CHUNKS;
    return std::max(PC_FOCK_POINTS, (per + 63) / 64 * 64);
}

extern "C" int mi_pc_fock_chunks(int npts, int64_t ld)
{
    (void)ld;   // the chunking depends on the points alone; the row stride is the caller's to size the scratch with
    if (npts <= 0) return 1;
    const int per = pc_fock_points(npts);
    return (npts + per - 1) / per;
}

// every coordinate, width and charge finite (one copy to the host: these entry points run once per geometry)
static int pc_check_points(const char *who, const double *d_pts, const double *d_q, int npts, hipStream_t st)
{
    std::vector<double> h((size_t)npts * 5);
    HIPCHK(hipMemcpyAsync(h.data(), d_pts, sizeof(double) * (size_t)npts * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h.data() + (size_t)npts * 4, d_q, sizeof(double) * (size_t)npts, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (size_t k = 0; k < h.size(); k++)
        if (!std::isfinite(h[k]))
            return fail("%s: %s %lld is not finite", who, k < (size_t)npts * 4 ? "coordinate or width of point" : "charge of point",
                        (long long)(k < (size_t)npts * 4 ? k / 4 : k - (size_t)npts * 4));
    return 0;
}

extern "C" int mi_pc_fock(mi_ctx *c, const double *d_pts, const double *d_q, int npts, double scale, int accumulate, double *d_work,
                          double *d_V, void *stream)
{
    if (!c || !d_pts || !d_q || !d_work || !d_V) return fail("mi_pc_fock: null argument");
    if (check_orbital_lmax(c, "mi_pc_fock")) return -1;
    if (npts < 0) return fail("mi_pc_fock: npts = %d", npts);
    if (npts == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    if (pc_check_points("mi_pc_fock", d_pts, d_q, npts, st)) return -1;
    PcArgs A{basis_dev(c)};
    const int64_t nn2 = (int64_t)c->nao * (c->nao + 1) / 2;
    A.pts = d_pts; A.q = d_q; A.npts = npts; A.ld = nn2 + (nn2 & 1); A.part = d_work;
    A.per = pc_fock_points(npts);
    A.nchunk = (npts + A.per - 1) / A.per;
    const int rc = launch_pair_classes<false>(c, A.nchunk, "mi_pc_fock", [&](auto la, auto lb, int first, int count) {
        PcArgs B = A;
        B.pairs = c->pair_classes[0].d_pairs + 2 * first;
        hipLaunchKernelGGL((pc_fock_kernel<decltype(la)::value, decltype(lb)::value>), dim3((unsigned)((int64_t)count * A.nchunk)), dim3(64),
                           0, st, B);
    });
    if (rc) return rc;
    const size_t nn = (size_t)c->nao * c->nao;
    hipLaunchKernelGGL(pcm_fock_finalize_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, st, d_work, A.nchunk, A.ld, c->nao, scale,
                       accumulate, d_V);
    HIPCHK(hipGetLastError());
    return 0;
}

// The gradient's chunking.  Point blocks: whole waves of sites, one site per lane for few sites and up to PC_GRAD_POINTS for
// many (apart = pairs x blocks x 24 B stays at pairs x 64 x 24 B until 32 768 sites).  Pair chunks: a budget for all classes of
// about 32 768 / blocks workgroups' worth, at most 1024, at most what keeps ppart = chunks x sites x 24 B within 128 MB, at
// least 64; every class gets a sixteenth of it, so that a class of few, expensive pairs (f f) is spread as widely as one of many
// cheap ones instead of running its pairs one after the other in a handful of workgroups.
struct PcGradPlan { int pblk, nblk, kpairs[16], chunk_start[17]; };

static PcGradPlan pc_grad_plan(const mi_ctx *c, int npts)
{
    PcGradPlan P;
    const mi_ctx::PairClasses &pc = c->pair_classes[1];
    P.pblk = std::min(PC_GRAD_POINTS, std::max(64, ((npts + 63) / 64 + 63) / 64 * 64));
    P.nblk = std::max(1, (npts + P.pblk - 1) / P.pblk);
    const int64_t by_memory = ((int64_t)1 << 27) / (24 * (int64_t)std::max(npts, 1));
    const int budget = (int)std::max<int64_t>(64, std::min<int64_t>({1024, 32768 / P.nblk, by_memory}));
    P.chunk_start[0] = 0;
    for (int k = 0; k < 16; k++) {
        const int count = pc.start[k + 1] - pc.start[k];
        P.kpairs[k] = std::max(1, (count + budget / 16 - 1) / (budget / 16));
        P.chunk_start[k + 1] = P.chunk_start[k] + (count + P.kpairs[k] - 1) / P.kpairs[k];
    }
    return P;
}

extern "C" int64_t mi_pc_grad_work(mi_ctx *c, int npts)
{
    if (!c || npts < 0) return fail("mi_pc_grad_work: bad arguments");
    const PcGradPlan P = pc_grad_plan(c, npts);
    return 3 * ((int64_t)c->pair_classes[1].start[16] * P.nblk + (int64_t)P.chunk_start[16] * npts);
}

extern "C" int mi_pc_grad(mi_ctx *c, const double *d_pts, const double *d_q, int npts, const double *d_D, double *d_work, double *d_grad_atoms,
                          double *d_grad_pts, void *stream)
{
    if (!c || !d_pts || !d_q || !d_D || !d_work || !d_grad_atoms || !d_grad_pts) return fail("mi_pc_grad: null argument");
    if (check_orbital_lmax(c, "mi_pc_grad")) return -1;
    if (npts < 0) return fail("mi_pc_grad: npts = %d", npts);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    if (npts == 0) {
        HIPCHK(hipMemsetAsync(d_grad_atoms, 0, sizeof(double) * 3 * (size_t)c->natm, st));
        return 0;
    }
    if (pc_check_points("mi_pc_grad", d_pts, d_q, npts, st)) return -1;
    const PcGradPlan P = pc_grad_plan(c, npts);
    const mi_ctx::PairClasses &pc = c->pair_classes[1];
    PcArgs A{basis_dev(c)};
    A.pts = d_pts; A.q = d_q; A.npts = npts; A.D = d_D; A.nblk = P.nblk; A.pblk = P.pblk;
    double *apart = d_work, *ppart = d_work + 3 * (int64_t)pc.start[16] * P.nblk;
    const int rc = launch_pair_classes<true>(c, P.nblk, "mi_pc_grad", [&](auto la, auto lb, int first, int count) {
        constexpr int K = decltype(la)::value * 4 + decltype(lb)::value;
        PcArgs B = A;
        B.pairs = pc.d_pairs + 2 * first;
        B.npair = count;
        B.kpairs = P.kpairs[K];
        B.apart = apart + 3 * (int64_t)first * P.nblk;
        B.ppart = ppart + 3 * (int64_t)P.chunk_start[K] * npts;
        const int64_t nwg = (int64_t)(P.chunk_start[K + 1] - P.chunk_start[K]) * P.nblk;
        hipLaunchKernelGGL((pc_grad_kernel<decltype(la)::value, decltype(lb)::value>), dim3((unsigned)nwg), dim3(64), 0, st, B);
    });
    if (rc) return rc;
    hipLaunchKernelGGL(pc_grad_atoms_kernel, dim3((unsigned)c->natm), dim3(256), 0, st, apart, pc.d_pairs, c->d_bas, pc.start[16], P.nblk,
                       d_grad_atoms);
    const int64_t n3 = 3 * (int64_t)npts;
    hipLaunchKernelGGL(pc_grad_points_kernel, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, st, ppart, P.chunk_start[16], n3, d_grad_pts);
    HIPCHK(hipGetLastError());
    return 0;
}

// =================================================================================================
// Determinant full CI inside an active space (mi_fci_*): gather / GEMM / gather over string link tables.
// =================================================================================================
#include "fci_kernels.h"

// =================================================================================================
// Closed-shell coupled cluster (mi_cc_*): the CCSD amplitude update and the (T) permutation / energy pass.
// =================================================================================================
#include "cc_kernels.h"

// =================================================================================================
// Restricted open-shell SCF (mi_rohf_fock): Roothaan's effective Fock operator, its orbital gradient and the gradient's norms.
// =================================================================================================
// Orbital classes in MO order: closed [0, ncore), open [ncore, ncore + nopen), virtual [ncore + nopen, nmo).  With Fc = (Fa + Fb) / 2
// the element (i, j) of F_eff is Fc inside a class and between closed and virtual, Fb between closed and open, Fa between open
// and virtual (PySCF's default Roothaan coefficients).  The inter-class elements are the ROHF orbital gradient; as the CDIIS
// error vector they take the sign of the occupation commutator F n - n F:  G[i][j] = sgn(class(i) - class(j)) F_eff[i][j].
// One thread per element and output (grid-stride over a fixed grid), plain loads and stores; sum |G|^2 and max |G| per workgroup
// by wave shuffles and a fixed-order pass over the waves, so the figures are bit-reproducible.
#define ROHF_BLOCKS 64

__global__ __launch_bounds__(256) void rohf_fock_kernel(const double *__restrict__ fa, const double *__restrict__ fb, int64_t ld, int ncore, int nopen,
                                                        int nmo, double *__restrict__ feff, double *__restrict__ g, double *__restrict__ part)
{
    __shared__ double red[4], redm[4];
    const size_t n = (size_t)nmo * nmo;
    const int nocc = ncore + nopen;
    double s = 0.0, m = 0.0;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (size_t)gridDim.x * blockDim.x) {
        const int i = (int)(idx / nmo), j = (int)(idx - (size_t)i * nmo);
        const int ci = (i >= ncore) + (i >= nocc), cj = (j >= ncore) + (j >= nocc);
        const size_t at = (size_t)i * ld + j;
        const double a = fa[at], b = fb[at];
        const int lo = ci < cj ? ci : cj, hi = ci < cj ? cj : ci;
        const double f = (lo == 0 && hi == 1) ? b : ((lo == 1 && hi == 2) ? a : 0.5 * (a + b));
        const double gv = ci > cj ? f : (ci < cj ? -f : 0.0);
        feff[at] = f;
        g[at] = gv;
        s += gv * gv;
        m = fmax(m, fabs(gv));
    }
    for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_down(m, off, 64));
    if ((threadIdx.x & 63) == 0) redm[threadIdx.x >> 6] = m;
    s = cc_block_sum(s, red);       // (its barriers also publish redm)
    if (threadIdx.x == 0) {
        part[blockIdx.x] = s;
        part[ROHF_BLOCKS + blockIdx.x] = fmax(fmax(redm[0], redm[1]), fmax(redm[2], redm[3]));
    }
}

extern "C" int mi_rohf_fock_blocks(void) { return ROHF_BLOCKS; }

extern "C" int mi_rohf_fock(const double *d_fa, const double *d_fb, int64_t ld, int ncore, int nopen, int nmo, double *d_feff, double *d_g,
                            double *d_part, void *stream)
{
    if (nmo < 1 || nmo > 46340 || ncore < 0 || nopen < 0 || (int64_t)ncore + nopen > nmo || ld < nmo)
        return fail("mi_rohf_fock: ncore = %d, nopen = %d, nmo = %d, ld = %lld", ncore, nopen, nmo, (long long)ld);
    if (!d_fa || !d_fb || !d_feff || !d_g || !d_part) return fail("mi_rohf_fock: bad argument");
    hipLaunchKernelGGL(rohf_fock_kernel, dim3(ROHF_BLOCKS), dim3(256), 0, (hipStream_t)stream, d_fa, d_fb, ld, ncore, nopen, nmo, d_feff, d_g, d_part);
    HIPCHK(hipGetLastError());
    return 0;
}
