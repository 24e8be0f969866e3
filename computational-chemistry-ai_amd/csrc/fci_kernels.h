// fci_kernels.h -- determinant full-CI kernels (mi_fci_*), included at the end of mi355scf.hip (same translation unit: fail(),
// HIPCHK).  Python side: mi355scf/fci.py builds the tables; DESIGN.md "Determinant FCI" has the algorithm and the accounting.
//
// Convention.  norb <= 16 spatial orbitals, (na, nb) electrons.  A string is an occupation bit mask (bit p = orbital p); the
// strings of one spin are numbered in ascending integer order.  The determinant |Ia Ib> is
//     a+_{i1,alpha} a+_{i2,alpha} ... a+_{j1,beta} a+_{j2,beta} ... |0>,    i1 < i2 < ...,  j1 < j2 < ...
// (all alpha creators, then all beta creators, ascending orbital order inside each spin).  With this order a same-spin pair
// a+_p a_q picks up the sign of its own string only: sign = (-1)^(occupied orbitals strictly between p and q).  CI vectors are
// FP64 [nvec][nsa][nsb], beta string fastest.
//
// Tables (host-built, device-resident, int32).  A link of string J is a single replacement a+_cre a_ann |J> = sgn |T>, ann
// occupied in J and cre empty in J or cre == ann; it is stored as the pair (ann * norb + cre, sgn * (T + 1)).
//     alink[nsa][nla][2]     the nla = na (norb - na) + na links of every alpha string, as a list
//     btab[norb^2][nsb]      the links of every beta string, dense: btab[ann * norb + cre][J] = sgn * (T + 1), 0 = no such link
// <J|E_rs|K> = <J|a+_r a_s|K> is non-zero exactly when J has the link (ann = r, cre = s) to K, with that sign -- so both gather
// directions below index D and F with the link's own `ann * norb + cre`, and no output element has two writers.
//
// Work arrays cover the alpha rows [a0, a0 + nrow) of every vector (ncol = nrow * nsb columns per vector) and have
// norb^2 + 1 planes: W[(plane * nvec + v) * ncol + (Ia - a0) * nsb + Ib].  Plane norb^2 of D is the vector itself, so that
// F = [ (pq|rs)/2 | h~_pq ] x D is ONE GEMM that already holds h~_pq c + G_pq.

#define FCI_MAX_NORB 16
#define FCI_NPT 13          /* sigma gather: beta strings per thread at 1024 threads; 13 * 1024 >= C(16, 8) = 12870 */

static int fci_threads(int nsb) { return nsb >= 1024 ? 1024 : std::max(64, (nsb + 63) / 64 * 64); }

// D[rs][v][J] = <J|E_rs|c_v> for the rows of the chunk (mode bit 0: alpha part, bit 1: beta part; 3 = spin-summed E_rs).
// One workgroup per (alpha row, vector).  The alpha part moves whole beta rows (coalesced); the beta part permutes inside the
// row, which is staged in LDS once and read from there.
__global__ __launch_bounds__(1024) void fci_gather_d_kernel(const double *__restrict__ c, int nsa, int nsb, int norb, int a0, int nvec,
                                                            const int *__restrict__ alink, int nla, const int *__restrict__ btab,
                                                            int mode, double *__restrict__ D)
{
    extern __shared__ double fci_lds[];
    double *row = fci_lds;                       // [nsb] the vector's own beta row
    int *amap = (int *)(fci_lds + nsb);          // [norb^2] alpha links of this row by (ann, cre)
    const int n2 = norb * norb, v = blockIdx.y, Ia = a0 + blockIdx.x;
    const size_t ncol = (size_t)gridDim.x * nsb, col0 = (size_t)blockIdx.x * nsb;
    const double *cv = c + (size_t)v * nsa * nsb;
    for (int i = threadIdx.x; i < n2; i += blockDim.x) amap[i] = 0;
    for (int i = threadIdx.x; i < nsb; i += blockDim.x) row[i] = cv[(size_t)Ia * nsb + i];
    __syncthreads();
    if (mode & 1)
        for (int l = threadIdx.x; l < nla; l += blockDim.x) {
            const int rs = alink[((size_t)Ia * nla + l) * 2];
            if ((unsigned)rs < (unsigned)n2) amap[rs] = alink[((size_t)Ia * nla + l) * 2 + 1];
        }
    __syncthreads();
    const int total = n2 * nsb;                  // <= 256 * 12870
    for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
        const int rs = idx / nsb, Ib = idx - rs * nsb;
        double val = 0.0;
        const int ta = amap[rs];
        if (ta) val = (ta > 0 ? 1.0 : -1.0) * cv[(size_t)(abs(ta) - 1) * nsb + Ib];
        if (mode & 2) {
            const int tb = btab[idx];
            if (tb) val += (tb > 0 ? 1.0 : -1.0) * row[abs(tb) - 1];
        }
        D[((size_t)rs * nvec + v) * ncol + col0 + Ib] = val;
    }
    for (int Ib = threadIdx.x; Ib < nsb; Ib += blockDim.x) D[((size_t)n2 * nvec + v) * ncol + col0 + Ib] = row[Ib];
}

// sigma[v][I] += sum_pq sum_{K in chunk} <I|E_pq|K> F[pq][v][K].  One workgroup per (alpha row of the WHOLE vector, vector):
// the alpha links of the row that end inside the chunk add whole beta rows of F; when the row itself is in the chunk, every
// plane of its F row is staged in LDS and permuted by the dense beta table.  Each thread owns its sigma elements (registers),
// so the accumulation over the chunks is a plain read-modify-write by successive launches on one stream.
__global__ __launch_bounds__(1024) void fci_gather_sigma_kernel(const double *__restrict__ F, int nsa, int nsb, int norb, int a0, int nrow,
                                                                int nvec, const int *__restrict__ alink, int nla,
                                                                const int *__restrict__ btab, double *__restrict__ sigma)
{
    extern __shared__ double fci_lds[];          // [nsb] one plane of this row of F
    const int n2 = norb * norb, v = blockIdx.y, Ia = blockIdx.x, T = blockDim.x;
    const size_t ncol = (size_t)nrow * nsb;
    double acc[FCI_NPT];
#pragma unroll
    for (int k = 0; k < FCI_NPT; ++k) acc[k] = 0.0;
    for (int l = 0; l < nla; ++l) {              // block-uniform
        const int pq = alink[((size_t)Ia * nla + l) * 2], t = alink[((size_t)Ia * nla + l) * 2 + 1];
        const int Ka = abs(t) - 1;
        if (Ka < a0 || Ka >= a0 + nrow) continue;
        const double s = t > 0 ? 1.0 : -1.0;
        const double *Fr = F + ((size_t)pq * nvec + v) * ncol + (size_t)(Ka - a0) * nsb;
#pragma unroll
        for (int k = 0; k < FCI_NPT; ++k) {
            const int Ib = threadIdx.x + k * T;
            if (Ib < nsb) acc[k] += s * Fr[Ib];
        }
    }
    if (Ia >= a0 && Ia < a0 + nrow) {            // block-uniform: the barriers below are reached by all or by none
        for (int pq = 0; pq < n2; ++pq) {
            const double *Fr = F + ((size_t)pq * nvec + v) * ncol + (size_t)(Ia - a0) * nsb;
            __syncthreads();
            for (int i = threadIdx.x; i < nsb; i += T) fci_lds[i] = Fr[i];
            __syncthreads();
            const int *bt = btab + (size_t)pq * nsb;
#pragma unroll
            for (int k = 0; k < FCI_NPT; ++k) {
                const int Ib = threadIdx.x + k * T;
                if (Ib < nsb) {
                    const int t = bt[Ib];
                    if (t) acc[k] += (t > 0 ? 1.0 : -1.0) * fci_lds[abs(t) - 1];
                }
            }
        }
    }
    double *sv = sigma + ((size_t)v * nsa + Ia) * nsb;
#pragma unroll
    for (int k = 0; k < FCI_NPT; ++k) {
        const int Ib = threadIdx.x + k * T;
        if (Ib < nsb) sv[Ib] += acc[k];
    }
}

// H_II = sum_{i in a} h_ii + sum_{i in b} h_ii + 1/2 [ sum_{i,j in a} (J_ij - K_ij) + sum_{i,j in b} (J_ij - K_ij) ] + sum_{i in a, j in b} J_ij,
// J_ij = (ii|jj), K_ij = (ij|ji).  One thread per determinant.
__global__ __launch_bounds__(256) void fci_hdiag_kernel(const double *__restrict__ h1, const double *__restrict__ jd, const double *__restrict__ kd,
                                                        int norb, const int *__restrict__ astr, int nsa, const int *__restrict__ bstr, int nsb,
                                                        double *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)nsa * nsb) return;
    const unsigned a = (unsigned)astr[i / nsb], b = (unsigned)bstr[i % nsb];
    double e = 0.0;
    for (int p = 0; p < norb; ++p) {
        const unsigned pa = (a >> p) & 1u, pb = (b >> p) & 1u;
        if (!(pa | pb)) continue;
        double jj = 0.0, kaa = 0.0, kbb = 0.0;
        for (int q = 0; q < norb; ++q) {
            const unsigned qa = (a >> q) & 1u, qb = (b >> q) & 1u;
            jj += (double)(qa + qb) * jd[p * norb + q];
            kaa += (double)qa * kd[p * norb + q];
            kbb += (double)qb * kd[p * norb + q];
        }
        e += (double)(pa + pb) * (h1[p * norb + p] + 0.5 * jj) - 0.5 * ((double)pa * kaa + (double)pb * kbb);
    }
    out[i] = e;
}

static int fci_check(const char *who, int norb, int nsa, int nsb, int a0, int nrow, int nvec, int nla)
{
    if (norb < 1 || norb > FCI_MAX_NORB) return fail("%s: norb = %d outside 1..%d", who, norb, FCI_MAX_NORB);
    if (nsa < 1 || nsb < 1 || nsb > FCI_NPT * 1024) return fail("%s: %d x %d strings (at most %d beta strings)", who, nsa, nsb, FCI_NPT * 1024);
    if (a0 < 0 || nrow < 1 || a0 + nrow > nsa) return fail("%s: alpha rows [%d, %d) outside [0, %d)", who, a0, a0 + nrow, nsa);
    if (nvec < 1 || nvec > 65535) return fail("%s: nvec = %d outside 1..65535", who, nvec);
    if (nla < 0 || nla > norb * norb) return fail("%s: %d alpha links per string", who, nla);
    return 0;
}

extern "C" int mi_fci_gather_d(const double *d_c, int nvec, int nsa, int nsb, int norb, int a0, int nrow, const int32_t *d_alink, int nla,
                               const int32_t *d_btab, int mode, double *d_D, void *stream)
{
    if (int rc = fci_check("mi_fci_gather_d", norb, nsa, nsb, a0, nrow, nvec, nla)) return rc;
    if (!d_c || !d_D || !d_btab || (nla > 0 && !d_alink) || mode < 1 || mode > 3) return fail("mi_fci_gather_d: bad argument");
    const size_t shm = sizeof(double) * nsb + sizeof(int) * norb * norb;
    if (shm > 64 * 1024)
        HIPCHK(hipFuncSetAttribute((const void *)fci_gather_d_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
    hipLaunchKernelGGL(fci_gather_d_kernel, dim3(nrow, nvec), dim3(fci_threads(nsb)), shm, (hipStream_t)stream, d_c, nsa, nsb, norb, a0, nvec,
                       d_alink, nla, d_btab, mode, d_D);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int mi_fci_gather_sigma(const double *d_F, int nvec, int nsa, int nsb, int norb, int a0, int nrow, const int32_t *d_alink, int nla,
                                   const int32_t *d_btab, double *d_sigma, void *stream)
{
    if (int rc = fci_check("mi_fci_gather_sigma", norb, nsa, nsb, a0, nrow, nvec, nla)) return rc;
    if (!d_F || !d_sigma || !d_btab || (nla > 0 && !d_alink)) return fail("mi_fci_gather_sigma: bad argument");
    const size_t shm = sizeof(double) * nsb;
    if (shm > 64 * 1024)
        HIPCHK(hipFuncSetAttribute((const void *)fci_gather_sigma_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
    hipLaunchKernelGGL(fci_gather_sigma_kernel, dim3(nsa, nvec), dim3(fci_threads(nsb)), shm, (hipStream_t)stream, d_F, nsa, nsb, norb, a0, nrow,
                       nvec, d_alink, nla, d_btab, d_sigma);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int mi_fci_hdiag(const double *d_h1, const double *d_jdiag, const double *d_kdiag, int norb, const int32_t *d_astr, int nsa,
                            const int32_t *d_bstr, int nsb, double *d_out, void *stream)
{
    if (norb < 1 || norb > FCI_MAX_NORB) return fail("mi_fci_hdiag: norb = %d outside 1..%d", norb, FCI_MAX_NORB);
    if (!d_h1 || !d_jdiag || !d_kdiag || !d_astr || !d_bstr || !d_out || nsa < 1 || nsb < 1) return fail("mi_fci_hdiag: bad argument");
    const size_t ndet = (size_t)nsa * nsb;
    hipLaunchKernelGGL(fci_hdiag_kernel, dim3((unsigned)((ndet + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_h1, d_jdiag, d_kdiag, norb,
                       d_astr, nsa, d_bstr, nsb, d_out);
    HIPCHK(hipGetLastError());
    return 0;
}
