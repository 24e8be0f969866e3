// cc_kernels.h -- closed-shell coupled-cluster kernels (mi_cc_*), included at the end of mi355scf.hip (same translation unit:
// fail(), HIPCHK).  Python side: mi355scf/ccsd.py; DESIGN.md "Coupled cluster" has the equations, the tiling and the byte counts.
//
// mi_cc_amp_update: one pass over the stacked residual [t1 (o v) | t2 (o o v v)] of a CCSD cycle.
// mi_cc_t_energy:   everything of the (T) correction after the GEMMs.  For an occupied triple (i, j, k) the driver leaves six raw
// cubes R_p[v][v][v], p = 0..5, R_p = X(pi_p(i, j, k)),
//     X(i, j, k)[a][b][c] = sum_d (ia|bd) t2[k][j][c][d] - sum_l (ia|lj) t2[l][k][b][c],
// pi_p the p-th permutation of three objects in lexicographic order (012, 021, 102, 120, 201, 210), and
//     W[x0][x1][x2] = sum_p R_p[x_{pi_p(0)}][x_{pi_p(1)}][x_{pi_p(2)}],                      x = (a, b, c)
//     V[a][b][c]    = W[a][b][c] + t1[i][a] (jb|kc) + t1[j][b] (ia|kc) + t1[k][c] (ia|jb)
//     E_ijk         = sum_abc (4 W_abc + W_bca + W_cab - 2 W_acb - 2 W_cba - 2 W_bac) V_abc / (3 D),   D = e_i + e_j + e_k - e_a - e_b - e_c
// (the form of (4 W_abc + W_bca + W_cab)(V_abc - V_cba) / (3 D) that is symmetric in i, j, k, so that i >= j >= k with weights suffices).
//
// Tiling.  The virtual range is cut into blocks of CC_TB = 8.  One workgroup owns an unordered block triple A >= B >= C and
// with it every ordered block position of that orbit (6, 3 or 1 distinct ones).  W on those positions needs exactly the
// tiles of the six raw cubes at those same positions, so every raw element is read once per launch, in its cube's own index
// order (rows of 8 doubles = 64 B).  Per raw cube the orbit's tiles are staged in LDS in native order; each thread then picks
// the permuted element of its own outputs from LDS and keeps W in registers (12 per thread).  W goes back to the same LDS
// tiles once, and the energy expression reads its six permuted neighbours from there.  Tiles have strides (73, 9, 1) doubles:
// the permuted reads put the lane-fastest local index on any of the three axes.

#define CC_TB 8
#define CC_SX 73
#define CC_SY 9
#define CC_TILE (CC_TB * CC_SX)
#define CC_AMP_MAX_BLOCKS 1024

__device__ __forceinline__ double cc_block_sum(double x, double *red)
{
    // fixed order: butterfly inside the wave, then the waves in ascending order
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) red[wave] = x;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < nw; ++w) s += red[w];
    __syncthreads();
    return s;       // valid in thread 0
}

// new = num / D, err = new - old, partial sums of |err|^2 and of the correlation energy of the NEW amplitudes
//     E = sum_ijab (t2[i][j][a][b] + t1[i][a] t1[j][b]) (2 (ia|jb) - (ib|ja))
__global__ __launch_bounds__(256) void cc_amp_update_kernel(const double *__restrict__ num, const double *__restrict__ told, double *__restrict__ tnew,
                                                            double *__restrict__ err, const double *__restrict__ ovov, const double *__restrict__ eo,
                                                            const double *__restrict__ ev, int o, int v, double *__restrict__ part)
{
    __shared__ double red[4];
    const size_t n1 = (size_t)o * v, n = n1 + n1 * n1, ov = (size_t)o * v;
    double s_dt = 0.0, s_e = 0.0;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (size_t)gridDim.x * blockDim.x) {
        double t;
        if (idx < n1) {
            const int i = (int)(idx / v), a = (int)(idx - (size_t)i * v);
            t = num[idx] / (eo[i] - ev[a]);
        } else {
            size_t r = idx - n1;
            const int b = (int)(r % v); r /= v;
            const int a = (int)(r % v); r /= v;
            const int j = (int)(r % o), i = (int)(r / o);
            t = num[idx] / (eo[i] + eo[j] - ev[a] - ev[b]);
            const double tia = num[(size_t)i * v + a] / (eo[i] - ev[a]), tjb = num[(size_t)j * v + b] / (eo[j] - ev[b]);
            const double g = 2.0 * ovov[((size_t)i * v + a) * ov + (size_t)j * v + b] - ovov[((size_t)i * v + b) * ov + (size_t)j * v + a];
            s_e += (t + tia * tjb) * g;
        }
        const double d = t - told[idx];
        tnew[idx] = t;
        err[idx] = d;
        s_dt += d * d;
    }
    const double a = cc_block_sum(s_dt, red), b = cc_block_sum(s_e, red);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = a;
        part[2 * blockIdx.x + 1] = b;
    }
}

__global__ void cc_amp_final_kernel(const double *__restrict__ part, int nblk, double *__restrict__ out)
{
    if (blockIdx.x == 0 && threadIdx.x < 2) {
        double s = 0.0;
        for (int b = 0; b < nblk; ++b) s += part[2 * b + threadIdx.x];
        out[threadIdx.x] = s;
    }
}

__host__ __device__ constexpr int cc_perm(int p, int m)
{
    // m-th entry of the p-th permutation of (0, 1, 2) in lexicographic order
    return m == 0 ? p / 2 : (m == 1 ? ((p & 1) ? (p / 2 == 2 ? 1 : 2) : (p / 2 == 0 ? 1 : 0)) : ((p & 1) ? (p / 2 == 0 ? 1 : 0) : (p / 2 == 2 ? 1 : 2)));
}
__host__ __device__ constexpr int cc_perm_index(int p0, int p1, int p2) { return 2 * p0 + (p1 > p2 ? 1 : 0); }
// pi_q after pi_p: entry m is pi_q(pi_p(m))
__host__ __device__ constexpr int cc_comp(int q, int p) { return cc_perm_index(cc_perm(q, cc_perm(p, 0)), cc_perm(q, cc_perm(p, 1)), cc_perm(q, cc_perm(p, 2))); }
static_assert(cc_perm(0, 0) == 0 && cc_perm(0, 1) == 1 && cc_perm(0, 2) == 2 && cc_perm(1, 0) == 0 && cc_perm(1, 1) == 2 && cc_perm(1, 2) == 1 &&
              cc_perm(2, 0) == 1 && cc_perm(2, 1) == 0 && cc_perm(2, 2) == 2 && cc_perm(3, 0) == 1 && cc_perm(3, 1) == 2 && cc_perm(3, 2) == 0 &&
              cc_perm(4, 0) == 2 && cc_perm(4, 1) == 0 && cc_perm(4, 2) == 1 && cc_perm(5, 0) == 2 && cc_perm(5, 1) == 1 && cc_perm(5, 2) == 0,
              "cc_perm: lexicographic permutations");
static_assert(cc_comp(0, 3) == 3 && cc_comp(3, 0) == 3 && cc_comp(3, 4) == 0 && cc_comp(1, 1) == 0 && cc_comp(3, 3) == 4, "cc_comp");

static int cc_t_nblocks(int v)
{
    const long nb = (v + CC_TB - 1) / CC_TB;
    return (int)(nb * (nb + 1) * (nb + 2) / 6);
}

__global__ __launch_bounds__(256) void cc_t_energy_kernel(const double *__restrict__ raw, int ntrip, int v, int o, const int *__restrict__ ijk,
                                                          const double *__restrict__ t1, const double *__restrict__ ovov, const double *__restrict__ eo,
                                                          const double *__restrict__ ev, double *__restrict__ part)
{
    __shared__ double tile[6 * CC_TILE];
    __shared__ double red[4];
    const int t = blockIdx.y;
    // blockIdx.x -> A >= B >= C
    int rem = blockIdx.x, A = 0;
    while (rem >= (A + 1) * (A + 2) / 2) { rem -= (A + 1) * (A + 2) / 2; ++A; }
    int B = 0;
    while (rem >= B + 1) { rem -= B + 1; ++B; }
    const int blk[3] = {A, B, rem};
    int bq[6][3], canon[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        bq[q][0] = blk[cc_perm(q, 0)]; bq[q][1] = blk[cc_perm(q, 1)]; bq[q][2] = blk[cc_perm(q, 2)];
        canon[q] = q;
#pragma unroll
        for (int r = q - 1; r >= 0; --r)
            if (bq[r][0] == bq[q][0] && bq[r][1] == bq[q][1] && bq[r][2] == bq[q][2]) canon[q] = r;
    }
    const size_t v3 = (size_t)v * v * v;
    int l[2][3];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int e = threadIdx.x + 256 * m;
        l[m][0] = e >> 6; l[m][1] = (e >> 3) & 7; l[m][2] = e & 7;
    }
    double acc[6][2];
#pragma unroll
    for (int q = 0; q < 6; ++q) acc[q][0] = acc[q][1] = 0.0;

#pragma unroll
    for (int p = 0; p < 6; ++p) {
        const double *cube = raw + ((size_t)p * ntrip + t) * v3;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            if (canon[r] != r) continue;                 // block-uniform
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const int gx = bq[r][0] * CC_TB + l[m][0], gy = bq[r][1] * CC_TB + l[m][1], gz = bq[r][2] * CC_TB + l[m][2];
                double val = 0.0;
                if (gx < v && gy < v && gz < v) val = cube[((size_t)gx * v + gy) * v + gz];
                tile[r * CC_TILE + l[m][0] * CC_SX + l[m][1] * CC_SY + l[m][2]] = val;
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            if (canon[q] != q) continue;
            const int r = canon[cc_comp(q, p)];
#pragma unroll
            for (int m = 0; m < 2; ++m)
                acc[q][m] += tile[r * CC_TILE + l[m][cc_perm(p, 0)] * CC_SX + l[m][cc_perm(p, 1)] * CC_SY + l[m][cc_perm(p, 2)]];
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        if (canon[q] != q) continue;
#pragma unroll
        for (int m = 0; m < 2; ++m) tile[q * CC_TILE + l[m][0] * CC_SX + l[m][1] * CC_SY + l[m][2]] = acc[q][m];
    }
    __syncthreads();

    const int i = ijk[3 * t], j = ijk[3 * t + 1], k = ijk[3 * t + 2];
    const double eijk = eo[i] + eo[j] + eo[k];
    const size_t ov = (size_t)o * v;
    double sum = 0.0;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        if (canon[q] != q) continue;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int a = bq[q][0] * CC_TB + l[m][0], b = bq[q][1] * CC_TB + l[m][1], c = bq[q][2] * CC_TB + l[m][2];
            if (a >= v || b >= v || c >= v) continue;
            double w[6];
#pragma unroll
            for (int s = 0; s < 6; ++s)
                w[s] = tile[canon[cc_comp(q, s)] * CC_TILE + l[m][cc_perm(s, 0)] * CC_SX + l[m][cc_perm(s, 1)] * CC_SY + l[m][cc_perm(s, 2)]];
            const double z = 4.0 * w[0] + w[3] + w[4] - 2.0 * (w[1] + w[2] + w[5]);
            const double vv = w[0] + t1[(size_t)i * v + a] * ovov[((size_t)j * v + b) * ov + (size_t)k * v + c]
                                   + t1[(size_t)j * v + b] * ovov[((size_t)i * v + a) * ov + (size_t)k * v + c]
                                   + t1[(size_t)k * v + c] * ovov[((size_t)i * v + a) * ov + (size_t)j * v + b];
            sum += z * vv / (3.0 * (eijk - ev[a] - ev[b] - ev[c]));
        }
    }
    const double s = cc_block_sum(sum, red);
    if (threadIdx.x == 0) part[(size_t)t * gridDim.x + blockIdx.x] = s;
}

__global__ __launch_bounds__(64) void cc_t_final_kernel(const double *__restrict__ part, int ntrip, int nblk, const double *__restrict__ wt,
                                                        double *__restrict__ et)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntrip) return;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += part[(size_t)t * nblk + b];
    et[t] = wt[t] * s;
}

extern "C" int mi_cc_amp_blocks(void) { return CC_AMP_MAX_BLOCKS; }

extern "C" int mi_cc_amp_update(const double *d_num, const double *d_told, double *d_tnew, double *d_err, const double *d_ovov, const double *d_eo,
                                const double *d_ev, int nocc, int nvir, double *d_part, double *d_out, void *stream)
{
    if (nocc < 1 || nvir < 1 || nocc > 4096 || nvir > 32768) return fail("mi_cc_amp_update: nocc = %d, nvir = %d", nocc, nvir);
    if (!d_num || !d_told || !d_tnew || !d_err || !d_ovov || !d_eo || !d_ev || !d_part || !d_out) return fail("mi_cc_amp_update: bad argument");
    const size_t n1 = (size_t)nocc * nvir, n = n1 + n1 * n1;
    const int nblk = (int)std::min<size_t>((n + 255) / 256, CC_AMP_MAX_BLOCKS);
    hipLaunchKernelGGL(cc_amp_update_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, d_num, d_told, d_tnew, d_err, d_ovov, d_eo, d_ev, nocc,
                       nvir, d_part);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(cc_amp_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, d_part, nblk, d_out);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int mi_cc_t_blocks(int nvir) { return nvir < 1 || nvir > 8192 ? 0 : cc_t_nblocks(nvir); }

extern "C" int mi_cc_t_energy(const double *d_raw, int ntrip, int nvir, int nocc, const int32_t *d_ijk, const double *d_wt, const double *d_t1,
                              const double *d_ovov, const double *d_eo, const double *d_ev, double *d_part, double *d_et, void *stream)
{
    if (nvir < 1 || nvir > 8192 || nocc < 1 || nocc > 4096) return fail("mi_cc_t_energy: nocc = %d, nvir = %d", nocc, nvir);
    if (ntrip < 1 || ntrip > 65535) return fail("mi_cc_t_energy: %d triples per launch (1..65535)", ntrip);
    if (!d_raw || !d_ijk || !d_wt || !d_t1 || !d_ovov || !d_eo || !d_ev || !d_part || !d_et) return fail("mi_cc_t_energy: bad argument");
    const int nblk = cc_t_nblocks(nvir);
    hipLaunchKernelGGL(cc_t_energy_kernel, dim3(nblk, ntrip), dim3(256), 0, (hipStream_t)stream, d_raw, ntrip, nvir, nocc, d_ijk, d_t1, d_ovov, d_eo,
                       d_ev, d_part);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(cc_t_final_kernel, dim3((ntrip + 63) / 64), dim3(64), 0, (hipStream_t)stream, d_part, ntrip, nblk, d_wt, d_et);
    HIPCHK(hipGetLastError());
    return 0;
}
