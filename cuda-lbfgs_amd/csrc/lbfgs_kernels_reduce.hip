// lbfgs_kernels_reduce.hip — the canonical fixed-order reduction on caller-owned
// device buffers: lbfgs_reducer_* of include/lbfgs_hip.h. A unit of its own beside
// the solver's device layer: it shares lbfgs_kernels_impl.h's wave_sum and group_tree, and nothing
// of the context.
//
// An objective evaluated on the device (LBFGS_OBJ_DEVICE) reduces its per-element terms to f with
// it, so that f is reproducible run to run and equals lbfgs_dev_dot's bits for the same data. The
// solver's own k_dot cannot be pointed at such a buffer: it loads whole 16-byte lane pairs of whole
// 128-element rows and relies on lbk_vec_alloc's zeroed padding behind element n - 1 and on its
// 256-byte alignment. k_reduce_segments keeps k_dot's element-to-lane mapping and accumulation
// order (segment s = [s L, min((s + 1) L, n)), wave w rows 4u + w, lane l elements 2l, 2l + 1 of a
// row, u ascending) and differs in two ways only:
//   - no element outside [0, n) is read: rows of a full segment lie inside it; the last, partial
//     segment is walked row by row with a test per element;
//   - any 8-byte alignment: 16-byte loads when both buffers are 16-byte aligned (a segment starts
//     at a multiple of 128 elements, a lane pair at an even element), two 8-byte loads otherwise.
// Then wave_sum, ((w0 + w1) + (w2 + w3)) = the segment partial, stored plainly; after the kernel
// boundary k_reduce_groups runs stage 2 (group_tree: 1024 partials per group, 0.0 beyond nseg),
// one workgroup per group, into a pinned host word per group; the host adds Q0 + ... + Q7 in order.
// Two launches, no atomics, no ticket, nothing waits on another workgroup.
#include "lbfgs_hip.h"
#include "lbfgs_kernels_impl.h"

namespace {

template <bool VEC, bool NT>
__device__ __forceinline__ double2 ld_pair(const double* p) {
    if (VEC) return ldv<NT>(p);
    double2 v;
    if (NT) {
        v.x = __builtin_nontemporal_load(p);
        v.y = __builtin_nontemporal_load(p + 1);
    } else {
        v.x = p[0];
        v.y = p[1];
    }
    return v;
}

// acc over one lane pair in the canonical order (element 0, then 1): fma for a dot; a plain add for
// a sum, which is the fma with 1.0 bit for bit
template <bool DOT>
__device__ __forceinline__ double acc_pair(double2 a, double2 b, double acc, bool v0, bool v1) {
    if (DOT) {
        if (v0) acc = fma(a.x, b.x, acc);
        if (v1) acc = fma(a.y, b.y, acc);
    } else {
        if (v0) acc = acc + a.x;
        if (v1) acc = acc + a.y;
    }
    return acc;
}

template <bool DOT, bool VEC, bool NT>
__global__ __launch_bounds__(LB_BLOCK) void k_reduce_segments(const double* __restrict__ a,
                                                              const double* __restrict__ b, int64_t n, int64_t L,
                                                              double* __restrict__ partials) {
    __shared__ double lds[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t sbeg = (int64_t)blockIdx.x * L;
    const int64_t len = min(L, n - sbeg);  // >= 1: the grid is nseg = ceil(n / L) workgroups
    const int nrow_tot = (int)((len + 127) / 128);
    const int nrows = nrow_tot > w ? (nrow_tot - w + 3) / 4 : 0;
    a += sbeg;
    if (DOT) b += sbeg;
    double acc = 0.0;
    int u = 0;
    if (len == L) {
        // a full segment: whole rows, all inside [0, n); 4 rows of loads in flight per lane
        for (; u + 4 <= nrows; u += 4) {
            double2 ra[4], rb[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t o = (int64_t)(4 * (u + j) + w) * 128 + 2 * lane;
                ra[j] = ld_pair<VEC, NT>(a + o);
                rb[j] = DOT ? ld_pair<VEC, NT>(b + o) : make_double2(0.0, 0.0);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = acc_pair<DOT>(ra[j], rb[j], acc, true, true);
        }
    }
    for (; u < nrows; ++u) {  // the rest, and the partial segment: a test per element
        const int64_t o = (int64_t)(4 * u + w) * 128 + 2 * lane;
        const bool v0 = o < len, v1 = o + 1 < len;
        double2 ra = make_double2(0.0, 0.0), rb = make_double2(0.0, 0.0);
        if (v1) {
            ra = ld_pair<VEC, NT>(a + o);
            if (DOT) rb = ld_pair<VEC, NT>(b + o);
        } else if (v0) {
            ra.x = a[o];
            if (DOT) rb.x = b[o];
        }
        acc = acc_pair<DOT>(ra, rb, acc, v0, v1);
    }
    acc = wave_sum(acc);
    if (lane == 0) lds[w] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

// stage 2 after the kernel boundary: workgroup g forms group g's tree (the solver's k_group_reduce
// arithmetic) and stores Q_g into the device slot and its pinned host mirror
__global__ __launch_bounds__(LB_BLOCK) void k_reduce_groups(const double* __restrict__ partials, int64_t nseg,
                                                            double* __restrict__ slot, double* hslot) {
    __shared__ double lds[4][1];
    const int g = (int)blockIdx.x;
    const int64_t gseg0 = (int64_t)g * LBK_SEG_PER_GROUP;
    group_tree<1, false>(partials, gseg0, gseg0, nseg, LBK_SEG_PER_GROUP, slot + g, hslot + g, lds);
}

// The same total of every row of a table in one launch (lbfgs_reduce_rows): within
// the batched solver's limits (n <= 32768: L = 512, at most 64 segments) a row is one workgroup's
// work and needs no second launch. Workgroup p takes row p; an inactive row's workgroup returns at
// once. The order is k_reduce_segments' for L = 512 followed by batch_pass's stage 2:
//   - segment s = [512 s, min(512 (s + 1), n)), wave w row w of it (128 elements), lane l elements
//     2l, 2l + 1 of that row; acc = 0.0, then fma(a.x, b.x, acc), fma(a.y, b.y, acc) for a dot,
//     acc + a.x, acc + a.y for a sum; an element at or beyond n contributes nothing;
//   - wave_sum; lane 0 of wave w leaves its value of segment s in LDS; the segment partial is
//     ((w0 + w1) + (w2 + w3));
//   - wave 0, lane j: the partial of segment j for j < nseg, else 0.0; wave_sum(p) + 0.0 is group 0
//     (the tree's levels above 64 add 0.0), and the 7 empty groups add 0.0 each; thread 0 stores.
// Nothing outside [0, n) of a row is read: full segments lie inside it and their loads are
// unconditional, four segments of them in flight per lane before the first wave_sum (accumulation
// stays per segment); the last, partial segment tests every element. 16-byte loads when this row's
// pointers are 16-byte aligned (with an odd lda the rows alternate), two 8-byte loads otherwise: a
// branch uniform in the workgroup. Plain cached loads: a row is at most 256 KiB and was just written.
template <bool DOT, bool VEC>
__device__ __forceinline__ void reduce_row_segments(const double* __restrict__ a, const double* __restrict__ b, int n,
                                                    double (&ws)[4][64]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nfull = n >> 9;
    const int o = w * 128 + 2 * lane;  // of this lane's pair within a segment
    int s = 0;
    for (; s + 4 <= nfull; s += 4) {
        double2 ra[4], rb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ra[j] = ld_pair<VEC, false>(a + (s + j) * 512 + o);
            rb[j] = DOT ? ld_pair<VEC, false>(b + (s + j) * 512 + o) : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double v = wave_sum(acc_pair<DOT>(ra[j], rb[j], 0.0, true, true));
            if (lane == 0) ws[w][s + j] = v;
        }
    }
    for (; s < nfull; ++s) {
        const double2 ra = ld_pair<VEC, false>(a + s * 512 + o);
        const double2 rb = DOT ? ld_pair<VEC, false>(b + s * 512 + o) : make_double2(0.0, 0.0);
        const double v = wave_sum(acc_pair<DOT>(ra, rb, 0.0, true, true));
        if (lane == 0) ws[w][s] = v;
    }
    if (n & 511) {  // the partial segment: a test per element
        const int i = s * 512 + o;
        const bool v0 = i < n, v1 = i + 1 < n;
        double2 ra = make_double2(0.0, 0.0), rb = make_double2(0.0, 0.0);
        if (v1) {
            ra = ld_pair<VEC, false>(a + i);
            if (DOT) rb = ld_pair<VEC, false>(b + i);
        } else if (v0) {
            ra.x = a[i];
            if (DOT) rb.x = b[i];
        }
        const double v = wave_sum(acc_pair<DOT>(ra, rb, 0.0, v0, v1));
        if (lane == 0) ws[w][s] = v;
    }
}

template <bool DOT>
__global__ __launch_bounds__(LB_BLOCK) void k_reduce_rows(const double* __restrict__ a, int64_t lda,
                                                          const double* __restrict__ b, int64_t ldb,
                                                          const int* __restrict__ active, int n,
                                                          double* __restrict__ out) {
    __shared__ double ws[4][64];  // [wave][segment]
    const int64_t p = blockIdx.x;
    if (active && active[p] == 0) return;
    a += p * lda;
    if (DOT) b += p * ldb;
    const uintptr_t bits = (uintptr_t)a | (DOT ? (uintptr_t)b : 0);
    if ((bits & 15) == 0)
        reduce_row_segments<DOT, true>(a, b, n, ws);
    else
        reduce_row_segments<DOT, false>(a, b, n, ws);
    __syncthreads();
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x, nseg = (n + 511) >> 9;
        const double q = lane < nseg ? (ws[0][lane] + ws[1][lane]) + (ws[2][lane] + ws[3][lane]) : 0.0;
        const double q0 = wave_sum(q) + 0.0;  // group 0: the tree's levels above 64 add 0.0
        if (lane == 0) {
            double tt = q0;
#pragma unroll
            for (int g = 1; g < LBK_GROUPS; ++g) tt = tt + 0.0;
            out[p] = tt;
        }
    }
}

}  // namespace

struct lbfgs_reducer {
    int64_t n, L, nseg;
    int device, nt;
    double* partials;  // [LBK_SEGS] segment partials (device)
    double* slot;      // [LBK_GROUPS] group values (device)
    double* hslot;     // their pinned host mirror, and its device address
    double* dhslot;
    hipStream_t stream;
};

extern "C" {

void lbfgs_reducer_destroy(lbfgs_reducer* r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    if (r->stream) (void)hipStreamSynchronize(r->stream);
    if (r->partials) (void)hipFree(r->partials);
    if (r->slot) (void)hipFree(r->slot);
    if (r->hslot) (void)hipHostFree(r->hslot);
    if (r->stream) (void)hipStreamDestroy(r->stream);
    delete r;
}

int lbfgs_reducer_create(lbfgs_reducer** out, int64_t n, int device) {
    if (!out) return LBFGS_ERR_BAD_ARG;
    *out = nullptr;
    lbk_geo G;
    if (n < 1 || device < 0 || lbk_geometry_plan(n, 0, 1, &G) != 0 || G.nseg > LBK_SEGS) return LBFGS_ERR_BAD_ARG;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device >= count) {
        (void)hipGetLastError();
        return LBFGS_ERR_HIP;
    }
    lbfgs_reducer* r = new (std::nothrow) lbfgs_reducer();
    if (!r) return LBFGS_ERR_NOMEM;
    r->n = n;
    r->L = G.L;
    r->nseg = G.nseg;
    r->device = device;
    // the solver's threshold for streaming loads past the Infinity Cache (lbk_create)
    r->nt = n * 8 > (88ll << 20) ? 1 : 0;
    if (hipSetDevice(device) != hipSuccess ||
        hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc((void**)&r->partials, sizeof(double) * LBK_SEGS) != hipSuccess ||
        hipMalloc((void**)&r->slot, sizeof(double) * LBK_GROUPS) != hipSuccess ||
        hipHostMalloc((void**)&r->hslot, sizeof(double) * LBK_GROUPS, hipHostMallocMapped | hipHostMallocCoherent) !=
            hipSuccess ||
        hipHostGetDevicePointer((void**)&r->dhslot, r->hslot, 0) != hipSuccess) {
        (void)hipGetLastError();
        lbfgs_reducer_destroy(r);
        return LBFGS_ERR_HIP;
    }
    *out = r;
    return 0;
}

int lbfgs_reducer_dot(lbfgs_reducer* r, const double* a_dev, const double* b_dev, void* hip_stream,
                      double* out_host) {
    if (!r || !a_dev || !out_host || ((uintptr_t)a_dev & 7) || ((uintptr_t)b_dev & 7)) return LBFGS_ERR_BAD_ARG;
    if (hipSetDevice(r->device) != hipSuccess) return LBFGS_ERR_HIP;
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : r->stream;
    const bool dot = b_dev != nullptr;
    const bool vec = (((uintptr_t)a_dev | (uintptr_t)b_dev) & 15) == 0;
    const dim3 grid((unsigned)r->nseg), block(LB_BLOCK);
#define LBR_LAUNCH(D, V, N) \
    hipLaunchKernelGGL((k_reduce_segments<D, V, N>), grid, block, 0, st, a_dev, b_dev, r->n, r->L, r->partials)
#define LBR_NT(D, V)           \
    do {                       \
        if (r->nt)             \
            LBR_LAUNCH(D, V, true);  \
        else                   \
            LBR_LAUNCH(D, V, false); \
    } while (0)
    if (dot && vec)
        LBR_NT(true, true);
    else if (dot)
        LBR_NT(true, false);
    else if (vec)
        LBR_NT(false, true);
    else
        LBR_NT(false, false);
#undef LBR_NT
#undef LBR_LAUNCH
    hipLaunchKernelGGL(k_reduce_groups, dim3(LBK_GROUPS), block, 0, st, r->partials, r->nseg, r->slot, r->dhslot);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        (void)hipGetLastError();
        return LBFGS_ERR_HIP;
    }
    double t = r->hslot[0];
    for (int g = 1; g < LBK_GROUPS; ++g) t = t + r->hslot[g];
    *out_host = t;
    return 0;
}

int lbfgs_reduce_rows(int device, int64_t n, int batch, const double* a_dev, int64_t lda, const double* b_dev,
                      int64_t ldb, const int* active_dev, double* out_dev, void* hip_stream) {
    // refusals first, before any HIP call: a machine without a device gives them too
    if (device < 0 || n < 1 || n > 32768 || batch < 1 || !a_dev || !out_dev || lda < n) return LBFGS_ERR_BAD_ARG;
    if (((uintptr_t)a_dev | (uintptr_t)b_dev | (uintptr_t)out_dev) & 7) return LBFGS_ERR_BAD_ARG;
    if (b_dev && ldb != 0 && ldb < n) return LBFGS_ERR_BAD_ARG;
    // the calling thread's device is left as it was (stateless: the caller may be torch on another one)
    int prev = device;
    if (hipGetDevice(&prev) != hipSuccess || (prev != device && hipSetDevice(device) != hipSuccess)) {
        (void)hipGetLastError();
        return LBFGS_ERR_HIP;
    }
    const hipStream_t st = (hipStream_t)hip_stream;
    const dim3 grid((unsigned)batch), block(LB_BLOCK);
    if (b_dev)
        hipLaunchKernelGGL(k_reduce_rows<true>, grid, block, 0, st, a_dev, lda, b_dev, ldb, active_dev, (int)n, out_dev);
    else
        hipLaunchKernelGGL(k_reduce_rows<false>, grid, block, 0, st, a_dev, lda, b_dev, ldb, active_dev, (int)n,
                           out_dev);
    const bool ok = hipGetLastError() == hipSuccess;
    if (prev != device) (void)hipSetDevice(prev);
    return ok ? 0 : LBFGS_ERR_HIP;
}

}  // extern "C"
