// lmi_nav_pop.h -- one step of the multi-level walk: the two pop kernels (queues in global memory / in LDS).  NOT a header of its own:
// lmi_mlp_fused.h includes it four times inside namespace lmi: with LMI_NAV_MASS 0 (nav_pop_kernel, nav_pop_lds_kernel: the walk as the
// reference runs it) and 1 (nav_pop_mass_kernel, nav_pop_lds_mass_kernel: the same walk with the path-mass stop of lmi_set_path_mass),
// each with LMI_NAV_ROWS 0 and 1 (nav_pop_rows_kernel, nav_pop_lds_rows_kernel, nav_pop_mass_rows_kernel, nav_pop_lds_mass_rows_kernel:
// the row-budget stop of lmi_set_stop_rows, alone and together with the path-mass stop).
//
// The mass forms: a recorded bucket's path mass -- read from pq_mass when the bucket is recorded -- goes into the query's running sum c
// (c_0 = m_0, c_j = c_{j-1} + m_j, binary32, in recording order), and the query goes on only while c < mass (false on NaN).  A stopped
// query writes nb into its out_len entry: every later step then takes it for finished (`have < nb`), so it pops nothing more and never
// queues for a model again; its remaining slots keep the -1 they were filled with.  (out_len is read by these kernels only.)  An
// internal pop leaves the entry's mass in parent_mass[q]: this step's mlp_fused_kernel<FM_NAV_MASS> multiplies the children's local
// probabilities by it.
//
// The rows forms: a recorded bucket with objects (cb >= 0) adds n(cb) -- one scattered 4-byte load from the index's live table -- to
// the query's int64 sum in acc[q]; a listed bucket without objects (-1) adds 0; the query goes on only while the sum is below `rows`,
// and stops the same way (nb into out_len).  With both stops a query goes on only while both conditions hold.
#if LMI_NAV_MASS && LMI_NAV_ROWS
#define LMI_NAV_POP nav_pop_mass_rows_kernel
#define LMI_NAV_POP_LDS nav_pop_lds_mass_rows_kernel
#define LMI_NAV_ARGS NavParams P, NavMass S, NavRows R
#elif LMI_NAV_ROWS
#define LMI_NAV_POP nav_pop_rows_kernel
#define LMI_NAV_POP_LDS nav_pop_lds_rows_kernel
#define LMI_NAV_ARGS NavParams P, NavRows R
#elif LMI_NAV_MASS
#define LMI_NAV_POP nav_pop_mass_kernel
#define LMI_NAV_POP_LDS nav_pop_lds_mass_kernel
#define LMI_NAV_ARGS NavParams P, NavMass S
#else
#define LMI_NAV_POP nav_pop_kernel
#define LMI_NAV_POP_LDS nav_pop_lds_kernel
#define LMI_NAV_ARGS NavParams P
#endif

__global__ __launch_bounds__(256) void LMI_NAV_POP(LMI_NAV_ARGS) {
    if (P.prev_active && *P.prev_active == 0) return;
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = q < P.nq;
    int have = live ? P.out_len[q] : P.nb;
#if LMI_NAV_MASS
    float cum = live ? S.cum[q] : 0.0f;
#endif
#if LMI_NAV_ROWS
    long long racc = live ? R.acc[q] : 0;
#endif
    const float* pp = P.pq_prob + (live ? q : 0);   // entry i at [i * nq]
    int* pe = P.pq_ent + (live ? q : 0);
    const int len = (live && have < P.nb) ? P.pq_len[q] : 0;
    // Bucket pops change nothing but the queue, so they continue within this step; the walk pauses at the first
    // internal node (its children's probabilities come from this step's grouped MLP launch) -- the same sequence
    // of pops as the reference's one-pop-per-iteration loop, in fewer launches.
    int my_cm = -1;
    while (len > 0) {
        float best = 0.0f;
        int bi = -1;
        for (int i = 0; i < len; ++i) {
            if (pe[(size_t)i * P.nq] < 0) continue;
            const float v = pp[(size_t)i * P.nq];
            if (bi < 0 || v >= best) { best = v; bi = i; }  // >=: the later entry wins a tie
        }
        if (bi < 0) break;  // queue exhausted: the remaining slots stay EMPTY (the reference would fail here)
        const int ent = pe[(size_t)bi * P.nq];
        pe[(size_t)bi * P.nq] = -1;
        const int cm = P.child_model[ent], cb = P.child_bucket[ent];
#if LMI_NAV_MASS
        if (cm >= 0) S.parent_mass[q] = S.pq_mass[(size_t)bi * P.nq + q];   // for this step's mlp_fused_kernel<FM_NAV_MASS>
#endif
        if (cm >= 0) { my_cm = cm; break; }
        if (cb >= -1) {
            P.out_slab[(size_t)q * P.nb + have] = cb;
            P.out_ent[(size_t)q * P.nb + have] = ent;
            P.out_len[q] = ++have;
            if (have >= P.nb) break;
#if LMI_NAV_MASS
            const float m = S.pq_mass[(size_t)bi * P.nq + q];   // one global load per pop: the masses need not live in LDS
            cum = have == 1 ? m : cum + m;
            S.cum[q] = cum;
            if (!(cum < S.mass)) { P.out_len[q] = P.nb; break; }   // stopped: every later step takes the query for finished
#endif
#if LMI_NAV_ROWS
            if (cb >= 0) { racc += R.nb_rows[cb]; R.acc[q] = racc; }   // cb < L: checked by the host before the walk (stop_rows_check)
            if (!(racc < R.rows)) { P.out_len[q] = P.nb; break; }      // stopped, as above
#endif
        }
    }
    nav_push(P, q, my_cm);
}

// The same step for trees whose queues fit LDS (cap <= NAV_LDS_CAP entries: [10, 10] has 110): a wave per 64 queries reads their queues
// ONCE (entry-major: a 256-byte row per entry) and every pop scans LDS instead of global memory -- a step's ~10 pops x up to 110
// entries per query took 43-101 us of a 0.96-ms walk at 10 000 queries (round 5 trace, profiles/r05_nav.txt); same pops, same order.
__global__ __launch_bounds__(64) void LMI_NAV_POP_LDS(LMI_NAV_ARGS) {
    extern __shared__ __attribute__((aligned(16))) char nav_smem[];
    if (P.prev_active && *P.prev_active == 0) return;
    float* sp = reinterpret_cast<float*>(nav_smem) + threadIdx.x;      // [cap][64]: this lane's column
    int* se = reinterpret_cast<int*>(nav_smem) + P.cap * 64 + threadIdx.x;
    const int q = blockIdx.x * 64 + threadIdx.x;
    const bool live = q < P.nq;
    int have = live ? P.out_len[q] : P.nb;
#if LMI_NAV_MASS
    float cum = live ? S.cum[q] : 0.0f;
#endif
#if LMI_NAV_ROWS
    long long racc = live ? R.acc[q] : 0;
#endif
    const int len = (live && have < P.nb) ? P.pq_len[q] : 0;
    const float* pp = P.pq_prob + (live ? q : 0);
    int* pe = P.pq_ent + (live ? q : 0);
    int mx = len;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o, 64));
    for (int i0 = 0; i0 < mx; i0 += 16) {   // 32 loads in flight per lane, then their LDS stores (clamped addresses: no branch per load)
        float v[16];
        int e[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const size_t o = (size_t)min(i0 + j, max(len - 1, 0)) * P.nq;
            v[j] = pp[o];
            e[j] = pe[o];
        }
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (i0 + j < len) { sp[(i0 + j) * 64] = v[j]; se[(i0 + j) * 64] = e[j]; }
    }
    int my_cm = -1;
    while (len > 0) {
        float best = 0.0f;
        int bi = -1;
        for (int i = 0; i < len; ++i) {
            const int e = se[i * 64];
            const float v = sp[i * 64];
            if (e >= 0 && (bi < 0 || v >= best)) { best = v; bi = i; }  // >=: the later entry wins a tie
        }
        if (bi < 0) break;
        const int ent = se[bi * 64];
        se[bi * 64] = -1;
        pe[(size_t)bi * P.nq] = -1;
        const int cm = P.child_model[ent], cb = P.child_bucket[ent];
#if LMI_NAV_MASS
        if (cm >= 0) S.parent_mass[q] = S.pq_mass[(size_t)bi * P.nq + q];   // for this step's mlp_fused_kernel<FM_NAV_MASS>
#endif
        if (cm >= 0) { my_cm = cm; break; }
        if (cb >= -1) {
            P.out_slab[(size_t)q * P.nb + have] = cb;
            P.out_ent[(size_t)q * P.nb + have] = ent;
            P.out_len[q] = ++have;
            if (have >= P.nb) break;
#if LMI_NAV_MASS
            const float m = S.pq_mass[(size_t)bi * P.nq + q];   // one global load per pop: the masses need not live in LDS
            cum = have == 1 ? m : cum + m;
            S.cum[q] = cum;
            if (!(cum < S.mass)) { P.out_len[q] = P.nb; break; }   // stopped: every later step takes the query for finished
#endif
#if LMI_NAV_ROWS
            if (cb >= 0) { racc += R.nb_rows[cb]; R.acc[q] = racc; }   // cb < L: checked by the host before the walk (stop_rows_check)
            if (!(racc < R.rows)) { P.out_len[q] = P.nb; break; }      // stopped, as above
#endif
        }
    }
    nav_push(P, q, my_cm);
}

#undef LMI_NAV_POP
#undef LMI_NAV_POP_LDS
#undef LMI_NAV_ARGS
