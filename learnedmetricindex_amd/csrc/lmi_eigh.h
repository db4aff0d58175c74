// lmi_eigh.h -- device code of lmi_eigh: the eigenvalues and eigenvectors of a symmetric binary64 matrix by the cyclic Jacobi method on
// the round-robin schedule of lmi_eigh_plan.h, bit for bit the same in either form and on any tile (include/lmi_hip.h states the
// arithmetic).  A round's output is a function of the round's input alone, element by element: eigh_rotation gives a
// pair's (c, s, t) from its three entries, eigh_b gives b_ij (i <= j) from the four entries at (i or its partner) x (j or its partner),
// eigh_step is the one plane rotation both use.  Both forms call exactly these, so no geometry can show.
//
// Resident form (eigh_resident_kernel, d <= RESIDENT_MAX_D): one block of 1024 threads holds A and V in LDS (the large allocation,
// up to 160 KB) for all sweeps.  A round is two phases split by barriers: D / 2 threads write the round's rotations to LDS; then every
// thread takes 2 x 2 blocks of A at (a row pair) x (a column pair) and (row, column pair) couples of V.  The four outputs of such a
// block depend on its own four inputs and the two rotations only, so a thread holds them in registers between its reads and its
// writes and the update happens where the data lies: one copy of A and V, no third barrier.
// Streamed form (eigh_round_kernel, one launch per round): A and V are double-buffered in device memory.  A block owns TILE row pairs x
// TILE column pairs of the round: it computes the 2 * TILE rotations it needs into LDS, then each thread loads its 2 x 2 block of A
// and stores the outputs and their mirrors.  Only tiles ti <= tj exist.  The blocks behind them do V: 2 * TILE rows x TILE column
// pairs, the column step alone.
// No matrix instruction: a round is d / 2 plane rotations, 6 flops per element moved; there is no product for v_mfma_f64 to take.
// Every operation of the contract goes through __dmul_rn / __dadd_rn / __dsub_rn / __ddiv_rn / __dsqrt_rn under contract(off).
#pragma once
#include <hip/hip_runtime.h>
#include "lmi_eigh_plan.h"

namespace lmi {

namespace ep = lmi_eigh_plan;

constexpr int EIGH_SKIPPED = 0, EIGH_ROTATED = 1, EIGH_BYE = 2;   // a pair's state; BYE: its q is >= d, p sits the round out

struct EighRot {
    double c, s, t;
    int state;
};

// the rotation of the pair with diagonal entries app, aqq and off-diagonal entry apq
__device__ __forceinline__ EighRot eigh_rotation(double app, double aqq, double apq) {
#pragma clang fp contract(off)
    EighRot r{1.0, 0.0, 0.0, EIGH_SKIPPED};
    const double fpp = fabs(app), fqq = fabs(aqq), fpq = fabs(apq);
    if (__dadd_rn(fpp, fpq) == fpp && __dadd_rn(fqq, fpq) == fqq) return r;
    const double theta = __ddiv_rn(__dsub_rn(aqq, app), __dmul_rn(2.0, apq));
    const double at = fabs(theta);
    if (at >= 0x1p512)   // theta * theta would overflow
        r.t = __ddiv_rn(1.0, __dmul_rn(2.0, theta));
    else
        r.t = __ddiv_rn(theta < 0.0 ? -1.0 : 1.0, __dadd_rn(at, __dsqrt_rn(__dadd_rn(__dmul_rn(theta, theta), 1.0))));
    r.c = __ddiv_rn(1.0, __dsqrt_rn(__dadd_rn(__dmul_rn(r.t, r.t), 1.0)));
    r.s = __dmul_rn(r.t, r.c);
    r.state = EIGH_ROTATED;
    return r;
}

// the new value at an index of a pair from the old value there (own) and at its partner (other); lower: the index is the pair's p
__device__ __forceinline__ double eigh_step(double own, double other, double c, double s, int state, bool lower) {
#pragma clang fp contract(off)
    if (state == EIGH_BYE) return own;
    return lower ? __dsub_rn(__dmul_rn(own, c), __dmul_rn(other, s)) : __dadd_rn(__dmul_rn(other, s), __dmul_rn(own, c));
}

// b_ij, i <= j.  pi, pj: the partners of i and j; ri, rj: the rotations of their pairs; a_ij, a_ipj, a_pij, a_pipj: A at
// (i, j), (i, pj), (pi, j), (pi, pj) -- those of a partner that sits out are not used.
__device__ __forceinline__ double eigh_b(int i, int j, int pi, int pj, const EighRot& ri, const EighRot& rj, double a_ij,
                                         double a_ipj, double a_pij, double a_pipj) {
#pragma clang fp contract(off)
    if (ri.state == EIGH_ROTATED) {
        if (j == pi) return 0.0;   // b_pq
        if (j == i) {              // b_pp = a_pp - t a_pq, b_qq = a_qq + t a_pq; pj == pi, so a_ipj is a_pq or its mirror
            const double ta = __dmul_rn(ri.t, a_ipj);
            return i < pi ? __dsub_rn(a_ij, ta) : __dadd_rn(a_ij, ta);
        }
    }
    const double u_ij = eigh_step(a_ij, a_ipj, rj.c, rj.s, rj.state, j < pj);
    if (ri.state == EIGH_BYE) return u_ij;
    const double u_pij = eigh_step(a_pij, a_pipj, rj.c, rj.s, rj.state, j < pj);
    return eigh_step(u_ij, u_pij, ri.c, ri.s, ri.state, i < pi);
}

// max |a_ij| over i <= j as a bit pattern (binary64 magnitudes order as integers; inf and NaN come out on top): *out starts at 0
__global__ __launch_bounds__(256) void eigh_absmax_kernel(const double* __restrict__ a, int d, unsigned long long* __restrict__ out) {
    unsigned long long best = 0;
    const long long total = (long long)d * d;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        if (idx / d > idx % d) continue;
        const unsigned long long b = __builtin_bit_cast(unsigned long long, a[idx]) & 0x7fffffffffffffffull;
        best = b > best ? b : best;
    }
    if (best) atomicMax(out, best);
}

// A = the mirror of a's upper triangle scaled by 2^(-e), V = I
__global__ __launch_bounds__(256) void eigh_init_kernel(const double* __restrict__ a, int d, int e, double* __restrict__ A,
                                                        double* __restrict__ V) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)d * d) return;
    const int i = (int)(idx / d), j = (int)(idx % d);
    A[idx] = ldexp(a[i <= j ? idx : (long long)j * d + i], -e);
    V[idx] = i == j ? 1.0 : 0.0;
}

// The 2 x 2 block of A at (the row pair X) x (the column pair Y), from Ain to Aout with its mirror: all that its four outputs depend on
// beside the two rotations.  In place (Ain == Aout) it is safe too: no other block reads or writes these eight places.
__device__ __forceinline__ void eigh_a_block(const double* Ain, double* Aout, int d, const int (&X)[2], const int (&Y)[2],
                                             const EighRot& rrow, const EighRot& rcol) {
    double m[2][2], out[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) m[a][b] = X[a] < d && Y[b] < d ? Ain[(size_t)X[a] * d + Y[b]] : 0.0;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int x = X[a], y = Y[b], px = X[1 - a], py = Y[1 - b];
            // the element is b_xy for x <= y; else the mirror of b_yx, whose four inputs are the mirrors of these four
            out[a][b] = x <= y ? eigh_b(x, y, px, py, rrow, rcol, m[a][b], m[a][1 - b], m[1 - a][b], m[1 - a][1 - b])
                               : eigh_b(y, x, py, px, rcol, rrow, m[a][b], m[1 - a][b], m[a][1 - b], m[1 - a][1 - b]);
        }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            if (X[a] >= d || Y[b] >= d) continue;
            Aout[(size_t)X[a] * d + Y[b]] = out[a][b];
            Aout[(size_t)Y[b] * d + X[a]] = out[a][b];
        }
}

// row i of V at the column pair Y: the column step alone
__device__ __forceinline__ void eigh_v_pair(const double* Vin, double* Vout, int d, int i, const int (&Y)[2], const EighRot& rcol) {
    const size_t row = (size_t)i * d;
    const double vp = Vin[row + Y[0]];
    if (rcol.state == EIGH_BYE) { Vout[row + Y[0]] = vp; return; }
    const double vq = Vin[row + Y[1]];
    Vout[row + Y[0]] = eigh_step(vp, vq, rcol.c, rcol.s, rcol.state, true);
    Vout[row + Y[1]] = eigh_step(vq, vp, rcol.c, rcol.s, rcol.state, false);
}

// a round's rotation of pair k, its two indices, and the OR into *rotated
__device__ __forceinline__ EighRot eigh_pair_rotation(const double* A, int d, int D, int r, int k, int* p, int* q, int* rotated) {
    ep::pair_of(D, r, k, p, q);
    EighRot rot{1.0, 0.0, 0.0, EIGH_BYE};
    if (*q < d) {
        const size_t pd = (size_t)*p * d, qd = (size_t)*q * d;
        rot = eigh_rotation(A[pd + *p], A[qd + *q], A[pd + *q]);
        if (rot.state == EIGH_ROTATED) *rotated = 1;   // the same value from every writer
    }
    return rot;
}

// dynamic LDS: ep::resident_lds_bytes(d).  status[0] = sweeps run, status[1] = 1 when the last of them rotated nothing.
__global__ __launch_bounds__(ep::RESIDENT_THREADS) void eigh_resident_kernel(const double* __restrict__ a, int d, int e,
                                                                              double* __restrict__ diag, double* __restrict__ Vout,
                                                                              int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char eigh_smem[];
    const int D = ep::even_d(d), H = D / 2, tid = threadIdx.x, dd = d * d;
    double* A = reinterpret_cast<double*>(eigh_smem);
    double* V = A + dd;
    double* rc = V + dd;   // the round's rotations, by pair
    double* rs = rc + H;
    double* rt = rs + H;
    int* st = reinterpret_cast<int*>(rt + H);
    int* ip = st + H;
    int* iq = ip + H;
    int* rotated = iq + H;

    for (int idx = tid; idx < dd; idx += ep::RESIDENT_THREADS) {
        const int i = idx / d, j = idx % d;
        A[idx] = ldexp(a[i <= j ? idx : j * d + i], -e);
        V[idx] = i == j ? 1.0 : 0.0;
    }
    if (tid == 0) *rotated = 0;
    __syncthreads();

    int sweeps = 0, converged = 0;
    while (sweeps < ep::SWEEP_CAP && !converged) {
        for (int r = 0; r < D - 1; ++r) {
            if (tid < H) {
                int p, q;
                const EighRot rot = eigh_pair_rotation(A, d, D, r, tid, &p, &q, rotated);
                rc[tid] = rot.c; rs[tid] = rot.s; rt[tid] = rot.t; st[tid] = rot.state; ip[tid] = p; iq[tid] = q;
            }
            __syncthreads();
            // every 2 x 2 block (kp <= kq) and every (row, pair) of V belongs to one thread and is updated where it lies
            for (int idx = tid; idx < H * H + d * H; idx += ep::RESIDENT_THREADS) {
                const bool is_a = idx < H * H;
                const int kp = is_a ? idx / H : 0, kq = is_a ? idx % H : (idx - H * H) % H;
                if (kp > kq) continue;
                const EighRot rcol{rc[kq], rs[kq], rt[kq], st[kq]};
                const int Y[2] = {ip[kq], iq[kq]};
                if (is_a) {
                    const EighRot rrow{rc[kp], rs[kp], rt[kp], st[kp]};
                    const int X[2] = {ip[kp], iq[kp]};
                    eigh_a_block(A, A, d, X, Y, rrow, rcol);
                } else {
                    eigh_v_pair(V, V, d, (idx - H * H) / H, Y, rcol);
                }
            }
            __syncthreads();
        }
        ++sweeps;
        converged = *rotated == 0;
        __syncthreads();
        if (tid == 0) *rotated = 0;   // the next write to it lies behind the barrier that follows
        __syncthreads();
    }
    for (int idx = tid; idx < dd; idx += ep::RESIDENT_THREADS) Vout[idx] = V[idx];
    for (int i = tid; i < d; i += ep::RESIDENT_THREADS) diag[i] = A[i * d + i];
    if (tid == 0) { status[0] = sweeps; status[1] = converged; }
}

// One round r of the streamed form: grid = a_tiles + v_row_tiles * tiles_side blocks of TILE * TILE threads.  *rotated is set to 1 by
// every block that finds a rotated pair (the same value from all: an OR).
template <int TILE>
__global__ __launch_bounds__(TILE * TILE) void eigh_round_kernel(const double* __restrict__ Ain, double* __restrict__ Aout,
                                                                 const double* __restrict__ Vin, double* __restrict__ Vout, int d,
                                                                 int r, int tiles_side, int a_tiles, int* __restrict__ rotated) {
    __shared__ double rc[2][TILE], rs[2][TILE], rt[2][TILE];
    __shared__ int st[2][TILE], ip[2][TILE], iq[2][TILE];   // st -1: no such pair (the tile runs past D / 2)
    const int D = ep::even_d(d), tx = threadIdx.x % TILE, ty = threadIdx.x / TILE;
    const bool is_a = (int)blockIdx.x < a_tiles;
    int ti, tj;
    if (is_a) {
        ep::tile_pair(tiles_side, (int)blockIdx.x, &ti, &tj);
    } else {
        ti = ((int)blockIdx.x - a_tiles) / tiles_side;   // a strip of 2 * TILE rows of V
        tj = ((int)blockIdx.x - a_tiles) % tiles_side;
    }
    if (threadIdx.x < 2 * TILE && (is_a || ty == 1)) {   // side 0: the row pairs (A only), side 1: the column pairs
        const int side = ty, k = (side ? tj : ti) * TILE + tx;
        int p = 0, q = 0;
        EighRot rot{1.0, 0.0, 0.0, -1};
        if (k < D / 2) rot = eigh_pair_rotation(Ain, d, D, r, k, &p, &q, rotated);
        rc[side][tx] = rot.c; rs[side][tx] = rot.s; rt[side][tx] = rot.t; st[side][tx] = rot.state;
        ip[side][tx] = p; iq[side][tx] = q;
    }
    __syncthreads();
    const EighRot rcol{rc[1][tx], rs[1][tx], rt[1][tx], st[1][tx]};
    if (rcol.state < 0) return;
    const int Y[2] = {ip[1][tx], iq[1][tx]};
    if (!is_a) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int i = (ti * TILE + ty) * 2 + h;
            if (i < d) eigh_v_pair(Vin, Vout, d, i, Y, rcol);
        }
        return;
    }
    const EighRot rrow{rc[0][ty], rs[0][ty], rt[0][ty], st[0][ty]};
    if (rrow.state < 0 || (ti == tj && ty > tx)) return;   // a diagonal tile: (ty, tx) and (tx, ty) hold the same elements
    const int X[2] = {ip[0][ty], iq[0][ty]};
    eigh_a_block(Ain, Aout, d, X, Y, rrow, rcol);
}

// order[rank] = i, rank = the eigenvalues before diag[i * stride]: the larger ones, and the equal ones of a lower index
__global__ __launch_bounds__(256) void eigh_order_kernel(const double* __restrict__ diag, long long stride, int d, int* __restrict__ order) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d) return;
    const double wi = diag[i * stride];
    int rank = 0;
    for (int j = 0; j < d; ++j) {
        const double wj = diag[j * stride];
        rank += wj > wi || (wj == wi && j < i);
    }
    order[rank] = i;
}

// block r < m: w[r] = diag[order[r]] * 2^e; v[r][.] = column order[r] of V, negated when its largest-magnitude entry (the lowest index
// on a tie) is negative
__global__ __launch_bounds__(256) void eigh_output_kernel(const double* __restrict__ diag, long long stride, const double* __restrict__ V,
                                                          const int* __restrict__ order, int d, int e, double* __restrict__ w,
                                                          double* __restrict__ v) {
    __shared__ double best_v[256];
    __shared__ int best_i[256];
    const int r = blockIdx.x, col = order[r], tid = threadIdx.x;
    double bv = -1.0;
    int bi = 0x7fffffff;
    for (int i = tid; i < d; i += 256) {   // ascending i: a strict > keeps the lowest index
        const double f = fabs(V[(size_t)i * d + col]);
        if (f > bv) { bv = f; bi = i; }
    }
    best_v[tid] = bv;
    best_i[tid] = bi;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h && (best_v[tid + h] > best_v[tid] || (best_v[tid + h] == best_v[tid] && best_i[tid + h] < best_i[tid]))) {
            best_v[tid] = best_v[tid + h];
            best_i[tid] = best_i[tid + h];
        }
        __syncthreads();
    }
    const bool neg = V[(size_t)(best_i[0] < d ? best_i[0] : 0) * d + col] < 0.0;   // (no entry compares: a column of NaN)
    for (int i = tid; i < d; i += 256) {
        const double x = V[(size_t)i * d + col];
        v[(size_t)r * d + i] = neg ? -x : x;
    }
    if (tid == 0) w[r] = ldexp(diag[col * stride], e);
}

}  // namespace lmi
