/*
 * lmi_hip.h -- C ABI of liblmi_hip.so: the MI355X (gfx950) implementation of the
 * LearnedMetricIndex query hot path.
 *
 * The reference (Coda-Research-Group/LearnedMetricIndex, pure Python) has no FFI of its own; its
 * native arithmetic is reached through two third-party Python calls.  Each entry point below
 * names the reference interface it replaces (paths relative to /root/reference/search/li/):
 *
 *   lmi_set_mlp / lmi_mlp_topk     NeuralNetwork.predict_proba            model.py:226-241
 *                                  (Sequential(Linear,ReLU,..)(x), softmax, topk)  model.py:45-49,97-99
 *                                  + _precompute_bucket_order 1-level     LearnedIndex.py:197-214
 *   lmi_mlp_proba                  NeuralNetwork.predict_proba (probabilities + full class order)
 *   lmi_buckets_*                  data_navigation.groupby(category_L*) + data_search.loc[...]
 *                                                                         LearnedIndex.py:101-104,350,357
 *   lmi_scan_topk                  the `for rank` x `for bucket` loop: filter_path_idxs, faiss.knn,
 *                                  1 - sim, local->global ids, stable merge
 *                                                                         LearnedIndex.py:107-146,328-373, utils.py:61-65
 *   lmi_search                     LearnedIndex.search (1-level index)    LearnedIndex.py:41-161
 *   lmi_knn_ip                     faiss.knn(xq, xb, k, METRIC_INNER_PRODUCT)   call site LearnedIndex.py:360-365
 *   lmi_merge_gathered             (no reference counterpart) merge of per-GPU top-k after the one
 *                                  RCCL all-gather of the bucket-sharded multi-GPU mode
 *
 * Conventions
 *   - Every function returns 0 on success and a negative code on failure; lmi_last_error()
 *     returns a thread-local, NUL-terminated description of the last failure.  Nothing throws.
 *   - A handle is bound to one device and one HIP stream (lmi_set_stream; default: the NULL
 *     stream).  All device work is enqueued on that stream.  A handle is not thread-safe.
 *   - `on_device` != 0: the float/int buffers of that call are device pointers valid on the
 *     handle's device and the call is asynchronous on the handle's stream.  `on_device` == 0: they
 *     are host pointers; the call copies in/out and returns after the results have landed.
 *   - All matrices are dense row-major.  Weights use torch.nn.Linear layout W[out][in].
 *   - Arithmetic contract (identical to oracle/lmi_oracle.c): every inner product is the k-ordered
 *     binary32 chain acc = fmaf(a[k], b[k], acc); Linear layers start the chain at the bias, the
 *     scan at 0.  Ties: lower class index / lower in-bucket row first; ranks merge by
 *     (distance, bucket rank, position) exactly like the reference's stable argsort.
 */
#ifndef LMI_HIP_H
#define LMI_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LMI_ABI_VERSION 1
#define LMI_API __attribute__((visibility("default")))
#define LMI_METRIC_IP 0 /* dist = 1 - <q,x> : the reference's only metric (LearnedIndex.py:360-368) */
#define LMI_METRIC_L2 1 /* dist = |q - x|^2, computed as |q|^2 - 2 (<q,x> - |x|^2/2); see lmi_set_metric */
#define LMI_K_PER_BUCKET 10 /* LearnedIndex.py:334: k is never forwarded to the bucket scan */
#define LMI_MAX_K 64
#define LMI_MAX_LAYERS 8

typedef struct lmi_index lmi_index;

/* Timing slots filled by lmi_timings (milliseconds; measured on the handle's stream by device-side clock stamps the kernels
 * write themselves -- lmi_set_timing 2, the default -- or by hipEvents between them -- levels 1 and 3). */
enum {
    LMI_T_INFERENCE = 0, /* MLP forward + class ranking   -> measured_time["inference"]            */
    LMI_T_ROUTE = 1,     /* routing (CSR of queries per bucket) + query packing                     */
    LMI_T_SCAN = 2,      /* the bucket scan (exact: scan_kernel; prefilter: slots 5+6+7) -> ["seq_search"] */
    LMI_T_MERGE = 3,     /* chunk/rank merge kernel       -> measured_time["sort"]                  */
    LMI_T_TOTAL = 4,     /* first to last event           -> measured_time["search"]                */
    LMI_T_PF_SAMPLE = 5, /* prefilter pass 1 (bounds from a sample); 0 in exact mode                */
    LMI_T_PF_EMIT = 6,   /* prefilter pass 2 (fp16 scan + candidate emission) -- the dominant kernel */
    LMI_T_RESCORE = 7,   /* select + exact re-rank of the survivors                                  */
    LMI_T_FALLBACK = 8,  /* exact brute-force fallback for overflowed slots (normally empty)         */
    LMI_T_CLOCK_MHZ = 9, /* NOT a time: the shader clock (MHz) the chip held under pass 2 -- block 0's life in s_memtime cycles over the
                            same in 100 MHz s_memrealtime ticks (timing level 2 only; 0 otherwise)             */
    LMI_T_COUNT = 12
};

LMI_API int lmi_abi_version(void);
LMI_API const char *lmi_last_error(void);
/* Provenance (no reference counterpart): "src=<sha256/16 of the library's sources this binary was built from> p2_waves=..
 * p2_bring=.. pf_cap=.." -- csrc/build.sh bakes the hash in (learnedmetricindex_amd/_srchash.py: every .h / .hip under csrc
 * and every .h under include); bench.py and profiles/summarize.py tie PMC summaries to the library that was really
 * LOADED with it (not to whatever sources lie in the working tree). */
LMI_API const char *lmi_build_info(void);

/* Lifetime. */
LMI_API int lmi_create(int device, lmi_index **out);
LMI_API int lmi_destroy(lmi_index *h);
LMI_API int lmi_set_stream(lmi_index *h, void *hip_stream);

/* MLP weights (host pointers).  dims[0] = input dim, dims[n_layers] = number of classes L;
 * W[i] is [dims[i+1]][dims[i]], b[i] is [dims[i+1]].  ReLU between layers, none after the last. */
LMI_API int lmi_set_mlp(lmi_index *h, int n_layers, const int *dims, const float *const *W,
                const float *const *b);

/* Which kernels run the navigation MLP: 2 = always the one-launch kernel of lmi_mlp_fused.h, 0 = always one kernel
 * per layer + ranking kernels, 1 (default) = the fused kernel when the batch has enough 32-query blocks to fill the
 * chip (and for predict_proba), the per-layer kernels for small batches.  All produce bit-identical logits, orders
 * and probabilities. */
LMI_API int lmi_set_fused_mlp(lmi_index *h, int mode);

/* Probability-mass stop of the 1-level navigation (no reference counterpart: the reference visits exactly n_buckets buckets
 * per query).  mass == 0 (default): off, every call behaves as without it.  0 < mass <= 1: in the bucket order that
 * lmi_mlp_topk, lmi_search and lmi_pipeline_submit compute, rank 0 is always visited and rank t >= 1 is visited iff
 * c_{t-1} < mass, where p_t is the probability lmi_mlp_proba returns at rank t (same maximum, same expf, row sum in class
 * order, one division), c_0 = p_0 and c_t = c_{t-1} + p_t, each a binary32 add with one rounding, taken in rank order;
 * the compare is binary32 and false on NaN.  A rank that is not visited gets bucket_order[q][t] = -1, which the scan and
 * the merge treat as an unvisited slot (dist = +inf, id = 0): kout and the output shapes do not change, n_buckets == 1
 * is unaffected.  Any other value (NaN included) is an error that leaves the setting as it was.  Per handle; a
 * lmi_clone_view copies its parent's value when it is made; may be changed between any two calls, the index is not
 * rebuilt.  lmi_mlp_proba and the multi-level calls (lmi_nav_order, lmi_search_tree) ignore it: the walk ranks by LOCAL
 * probabilities, whose running sum is not a covered probability; the walk's own stop is lmi_set_path_mass below, which
 * accounts in path probabilities.  All three ranking paths (lmi_set_fused_mlp) give bit-identical orders. */
LMI_API int lmi_set_stop_mass(lmi_index *h, float mass);

/* Probability-mass stop of the multi-level walk (lmi_nav_order, lmi_search_tree; no reference counterpart).  The product of
 * the local probabilities along a path is a distribution over the leaves, so the walk can account for how much of it the
 * buckets it has recorded cover -- without changing its order: priorities (the local probability), pop order and tie rule
 * (the later-pushed entry wins; the root's children are pushed least probable first) stay the reference's.
 * Every queue entry carries a path mass m beside its priority: a root child has m = p, the probability lmi_mlp_proba
 * returns for it; a child pushed when an internal entry of mass M is expanded has m = M * p_local, one binary32 multiply,
 * rounded before anything is added to it.  When the walk records a bucket of mass m -- a listed bucket without objects
 * (child_bucket -1) included; a dropped path (-2) is not recorded and adds nothing -- c_0 = m_0 and c_j = c_{j-1} + m_j in
 * recording order, each a binary32 add.  The first bucket is always recorded; after j recorded buckets the query goes on
 * popping only while c_{j-1} < mass (a binary32 compare, false on NaN).  A stopped query pops nothing more and never
 * queues for a model again; its remaining slab_ids / entries slots stay -1, which lmi_scan_topk treats as unvisited
 * (dist = +inf, id = 0): kout and the output shapes do not change, n_buckets == 1 is unaffected.
 * mass == 0 (default): off, the walk runs the same kernels as without the setting.  Any value outside [0, 1] (NaN
 * included) is an error that leaves the setting as it was.  Per handle; a lmi_clone_view copies its parent's value when it
 * is made; may be changed between any two calls.  Independent of lmi_set_stop_mass: the 1-level calls (lmi_mlp_topk,
 * lmi_search, lmi_pipeline_submit, lmi_mlp_proba) ignore this setting, the walk ignores that one. */
LMI_API int lmi_set_path_mass(lmi_index *h, float mass);

/* Row-budget stop (no reference counterpart in code; the LMI literature states its search budget this way: "stop after the
 * visited buckets hold 1 % of the dataset").  A query visits buckets in the model's order until the buckets it has visited
 * hold `rows` objects or more.  n(b) is the number of objects the handle's index holds in slab bucket b at the time of the
 * CALL -- what lmi_bucket_sizes returns; the kernels read it from the index's device table, so it is live, not a snapshot
 * taken when the setter ran: after lmi_buckets_insert / lmi_buckets_delete the next call cuts by the new counts.
 * rows == 0 (default): off, every call launches exactly the kernels it launches without the setting.  rows < 0: an error
 * that leaves the setting as it was.
 * 1-level calls (lmi_mlp_topk, lmi_search, lmi_search_f16, lmi_pipeline_submit): in the bucket order r_0 = n(class_0) and
 * r_t = r_{t-1} + n(class_t), summed in int64; a rank whose class is -1 (the NaN case of the ranking) adds 0.  Rank 0 is
 * always visited, rank t >= 1 is visited iff r_{t-1} < rows.  A rank that is not visited gets bucket_order[q][t] = -1,
 * which the scan and the merge treat as an unvisited slot.  The bucket that crosses the budget is scanned whole: there are
 * no partial buckets.  n >= 0, so the sum never decreases and the first cut rank ends the order.
 * Walk calls (lmi_nav_order, lmi_search_tree, lmi_search_tree_f16): order, priorities and tie rule are untouched.  When
 * the walk records a bucket, r_j = r_{j-1} + n(child_bucket); a listed bucket without objects (child_bucket -1) adds 0, a
 * dropped path (-2) is not recorded and adds nothing.  The first bucket is always recorded; after j recorded buckets the
 * query goes on popping only while r_{j-1} < rows.  A stopped query pops nothing more and never queues for a model again;
 * its remaining slab_ids / entries slots stay -1.
 * Together with the other stops: with lmi_set_stop_mass on a 1-level call, or lmi_set_path_mass on a walk call, the query
 * goes on only while BOTH conditions hold; both are prefix cuts of the same order, so a query visits the smaller of the two
 * counts.  (lmi_set_stop_mass stays without effect on the walk and lmi_set_path_mass on the 1-level calls.)
 * Not affected: n_buckets == 1 is never cut, lmi_mlp_proba is never cut, lmi_scan_topk on a caller's own bucket order is
 * unchanged, kout and all output shapes are unchanged.
 * Refused before any launch when rows > 0 and n_buckets > 1: a handle without a built index (lmi_mlp_topk on a handle
 * that only has an MLP keeps working with the stop off); an index built with an `owned` mask that leaves a bucket out (a
 * sharded rank does not know the other ranks' counts, and ranks that cut differently would merge wrong results); a 1-level
 * call whose model has more classes than the index has bucket ids (for the walk: a child_bucket that is no bucket id of
 * the index).  Each message names the condition.
 * Per handle; a lmi_clone_view copies its parent's value when it is made; lmi_subset hands it on, and the subset cuts by
 * its OWN counts; may be changed between any two calls, the index is not rebuilt. */
LMI_API int lmi_set_stop_rows(lmi_index *h, int64_t rows);

/* Multi-level index (len(n_categories) > 1; LearnedIndex.py:216-325, PriorityQueue.py:18-94): the models of
 * the internal nodes and the tree.  Model 0 is the root (lmi_set_mlp); lmi_nav_set_model sets model_id >= 1
 * (arguments as lmi_set_mlp).  lmi_nav_set_tree: child e = child_offset[m] + c is class c of model m:
 * child_model[e] >= 1 -> that internal node's model, -1 -> a leaf; child_bucket[e] >= 0 -> slab bucket id
 * (the bucket ids of lmi_buckets_begin), -1 -> a bucket path that holds no object (LearnedIndex.bucket_paths
 * lists it: it is recorded and its slot stays unvisited), -2 -> not a bucket (the popped path is dropped, as
 * the reference's _visit_buckets does).
 * lmi_nav_order: the batched priority-queue walk on the device -- every query pops its most probable entry
 * (priority = the child's LOCAL softmax probability; ties: the entry pushed later), internal nodes
 * are expanded by their model for all queries that popped them (one grouped launch per step), until nb
 * buckets are recorded.  slab_ids[nq][nb], entries[nq][nb] (flat child index of each visited bucket; -1 where
 * the queue ran out). */
LMI_API int lmi_nav_set_model(lmi_index *h, int model_id, int n_layers, const int *dims, const float *const *W,
                      const float *const *b);
LMI_API int lmi_nav_set_tree(lmi_index *h, int n_models, const int32_t *child_offset, const int32_t *child_model,
                     const int32_t *child_bucket);
LMI_API int lmi_nav_order(lmi_index *h, const float *queries_nav, int nq, int nb, int32_t *slab_ids,
                  int32_t *entries, int on_device);

/* LearnedIndex.search for a multi-level index in ONE call (reference: search/li/LearnedIndex.py:41-83 the entry point, :216-325 the walk,
 * :328-373 the bucket scans): lmi_nav_order followed by lmi_scan_topk on the walk's buckets, without the host in between.  Arguments as
 * lmi_search (queries_nav [nq][model inputs], queries_search [nq][d]; dists / ids / keys [nq][kout]); slab_ids / entries: nullable
 * [nq][nb] outputs of the walk (as lmi_nav_order).  With host buffers the scan vectors are uploaded on a library-owned stream while the
 * walk runs.  Trees of up to 16 models run without any host round trip inside the call. */
LMI_API int lmi_search_tree(lmi_index *h, const float *queries_nav, const float *queries_search, int nq, int nb, int k,
                    float *dists, uint32_t *ids, uint32_t *keys, int32_t *slab_ids, int32_t *entries, int on_device);

/* Metric of the bucket scan (call before lmi_buckets_begin; default LMI_METRIC_IP).  The reference scans with
 * faiss.METRIC_INNER_PRODUCT only (LearnedIndex.py:364); LMI_METRIC_L2 is what faiss.knn(..., METRIC_L2) would be in
 * its place: squared Euclidean distances, ascending.  Canonical arithmetic (oracle/lmi_oracle.c:lmi_oracle_knn_l2):
 * with the k-ordered fmaf chains s = <q,x>, xn = <x,x>, qn = <q,q>:  key = s + (-xn/2)  (one rounding),
 * dist = fmaf(-2, key, qn);  neighbours by key descending, ties -> lower row; short buckets are padded with
 * FLT_MAX.  Internally every stored vector carries the column -xn/2 (lmi_bucket_read does not return it). */
LMI_API int lmi_set_metric(lmi_index *h, int metric);

/* How a built index keeps its scan vectors (call before lmi_buckets_begin, like lmi_set_metric: the value takes effect at the next
 * lmi_buckets_begin; default LMI_STORAGE_F32).  No reference counterpart (the reference keeps the DataFrame).
 *   LMI_STORAGE_F32  a row-major f32 image (exact re-rank, fallback, read-back, mutation) + the prefilter's fp16 fragments.
 *   LMI_STORAGE_F16  the fp16 fragments ONLY: a third of the device memory, for vectors that are binary16-exact (data distributed
 *                    as 16-bit floats; lmi_buckets_add_rows_f16 takes it as such).  lmi_buckets_add_rows / _add_owned_rows take f32
 *                    rows; each piece is converted as it arrives and no f32 image of more than the staged piece ever exists.  The LIBRARY decides, on the device, whether
 *                    the data is admissible: every stored x is finite and exactly representable in binary16 (subnormals included),
 *                    and so is x * s for the index scale s (the power of two with max|x| * s in [0.5, 1); only a scale below 1, i.e.
 *                    max|x| >= 1, can lose bits).  Inadmissible data: lmi_buckets_end fails, the message names the condition, and the
 *                    handle is left without an index (lmi_buckets_begin may be called again) -- nothing approximate is ever served.
 *                    Widening a half and undoing a power-of-two scale are exact, so every search returns bit for bit what
 *                    LMI_STORAGE_F32 returns for the same rows, and lmi_bucket_read returns the original f32 rows.  The exact
 *                    re-rank gathers a survivor's row from 16-byte fragment pieces instead of one contiguous row: that is the price.
 *                    Refused with LMI_STORAGE_F16 (the handle stays as it was): LMI_METRIC_L2 (the -|x|^2/2 column is not
 *                    fp16-exact), lmi_set_prefilter(0) (the all-f32 scan needs f32 fragments), a device whose fp16 self-test
 *                    failed, and lmi_buckets_insert / lmi_buckets_delete -- mutation of a compact index is a follow-up.
 * Any other value is an error.  lmi_knn_ip keeps an LMI_STORAGE_F32 index of its own. */
#define LMI_STORAGE_F32 0
#define LMI_STORAGE_F16 1
LMI_API int lmi_set_storage(lmi_index *h, int storage);
/* Device bytes of the index images the handle holds at this moment: the vector images, the ids and the per-bucket tables -- not the
 * per-call workspaces, not the ingest staging.  Valid from lmi_buckets_begin on (a clone view reports its parent's images). */
LMI_API int lmi_index_bytes(lmi_index *h, int64_t *bytes);

/* Bucket-contiguous index in HBM.
 * begin: labels[N] = data_prediction[:,0] (bucket of every object, 0 <= label < L), ids[N] = the
 *        DataFrame index labels (NULL -> 1..N, search.py:190-191), owned[L] = which buckets this
 *        handle keeps (NULL -> all; used by the bucket-sharded multi-GPU mode).  Host pointers.
 *        L < 2^20 (any fan-out the reference's n_categories can name in practice, e.g. [100, 100]).
 * add_rows: rows [nrows][d] are the original objects row0 .. row0+nrows-1 (any order of calls, each
 *        object exactly once); they are scattered to their bucket-contiguous position on device.
 * end:   finishes the build.  The built index can then be changed in place by lmi_buckets_insert / lmi_buckets_delete. */
LMI_API int lmi_buckets_begin(lmi_index *h, int64_t N, int d, int L, const int64_t *labels,
                      const uint32_t *ids, const uint8_t *owned);
LMI_API int lmi_buckets_add_rows(lmi_index *h, const float *rows, int64_t row0, int64_t nrows, int on_device);
/* Owned-only ingest (bucket-sharded ranks): rows [nrows][d] are the objects index[0..nrows) (original row
 * numbers, each OWNED object exactly once, any order); objects of buckets this handle does not own are never
 * passed in, so a rank of an 8-way shard reads 1/8 of the dataset.  Not to be mixed with lmi_buckets_add_rows
 * within one build.  `on_device` covers both pointers. */
LMI_API int lmi_buckets_add_owned_rows(lmi_index *h, const float *rows, const int64_t *index, int64_t nrows,
                               int on_device);
LMI_API int lmi_buckets_end(lmi_index *h);
/* Mutation of a built index (no reference counterpart: the reference rebuilds).  rows [nrows][d] (host, or device with
 * on_device), labels [nrows] bucket ids in [0, L) (host), ids [nrows] (host; NULL -> an error, ids are the caller's).
 * Objects of buckets this handle does not own (lmi_buckets_begin's `owned`) are skipped; *n_stored (nullable) <- stored.
 * Each inserted object goes after the last object of its bucket. */
LMI_API int lmi_buckets_insert(lmi_index *h, const float *rows, const int64_t *labels, const uint32_t *ids, int64_t nrows,
                               int on_device, int64_t *n_stored);
/* Removes every object whose id is in ids[n] (host); the survivors keep their order.  *n_removed (nullable) <- removed
 * (ids not present are not an error).
 * Both calls: searches then return exactly what a fresh lmi_buckets_begin / add_rows / end of the equivalent object list
 * returns (the survivors in the order the index held them, then the inserted objects in call order).  They synchronise
 * the handle's stream first (a search enqueued before reads the index as it was) and return when the index is updated.
 * Refused, with the index unchanged, when the index is not built, when a lmi_clone_view of the handle is alive (or the
 * handle is one), when a label is outside [0, L) or when rows, spare row-blocks and holes would pass the 32-bit positions
 * of the slab; a slab that must grow is copied into new allocations, so a failed allocation leaves the old index. */
LMI_API int lmi_buckets_delete(lmi_index *h, const uint32_t *ids, int64_t n, int64_t *n_removed);
/* A filtered copy of a built index, derived on the device (no reference counterpart: the reference filters its DataFrames and
 * rebuilds).  ids[n] (host) lists the objects the new index holds (LMI_SUBSET_KEEP) or leaves out (LMI_SUBSET_DROP); ids that are
 * not present and duplicates are ignored; *n_kept (nullable) <- the objects the new index holds.  LMI_SUBSET_DROP with n == 0 is the
 * full copy, LMI_SUBSET_KEEP with n == 0 the index of zero objects.
 * *out is a NEW, INDEPENDENT handle on h's device: it owns copies of the root model, the node models, the tree tables and its own
 * index images -- nothing is borrowed (it is no clone view and does not count as one), h may be destroyed before it, and either may
 * be rebuilt or mutated without the other noticing.  It carries h's settings: metric, storage, prefilter on or off,
 * lmi_set_fused_mlp, lmi_set_stop_mass, lmi_set_path_mass, lmi_set_stop_rows, the timing level and the `owned` mask of a sharded rank; a chunk length
 * fixed by lmi_set_chunk_rows stays fixed, otherwise it is chosen as lmi_buckets_begin chooses it, for the subset's own size.  Its
 * stream is the NULL stream until lmi_set_stream.
 * The new handle holds exactly what lmi_create + those settings + lmi_buckets_begin / add_rows / end would hold for the object list
 * "every bucket's kept objects, in the order h holds them": every search returns the same dists, ids and keys bit for bit,
 * lmi_bucket_sizes / lmi_bucket_read / lmi_bucket_read_f16 / lmi_index_bytes return the same, and lmi_debug_layout shows a fresh
 * build's layout with all four counters zero -- the slack, relocated buckets and holes of a mutated h do not survive, so the full copy
 * is also h's compaction.  An LMI_STORAGE_F16 index, which lmi_buckets_delete refuses, loses objects this way without any binary32
 * image: the kept halves are moved as stored and brought to the subset's own scale by an exact power of two.  An owned bucket that is
 * left empty no longer counts as holding rows on some rank (lmi_buckets_delete's rule); buckets of other ranks keep h's word.
 * The call synchronises h's stream first, only READS h -- so it is allowed while clone views of h live, and on a clone view -- and
 * returns when the new index is complete.  Peak device memory: h's images + the subset's + 8 bytes per slab row of h (the keep and
 * source maps, freed before the call returns).
 * Refused, with *out left NULL and h untouched: h is not built or is being built, an unknown mode, n < 0, n > 0 with NULL ids, NULL
 * out.  A failed allocation frees whatever the call allocated; the message says how many bytes it wanted. */
#define LMI_SUBSET_KEEP 0   /* ids lists the objects the new index holds      */
#define LMI_SUBSET_DROP 1   /* ids lists the objects the new index leaves out */
LMI_API int lmi_subset(lmi_index *h, const uint32_t *ids, int64_t n, int mode, lmi_index **out, int64_t *n_kept /* nullable */);
/* A re-bucketed copy of a built index, derived on the device (no reference counterpart: the reference re-labels its DataFrames and
 * rebuilds).  lmi_subset is "same labels, fewer objects"; this is "same objects, new labels, any new L".
 * The new label of a stored object: labels[i] if its id is ids[i] (host arrays, n entries, every id listed once); otherwise
 * bucket_map[its bucket] (host, [L of h]; NULL: the identity, which needs L_new >= L).  A map entry of -1 says "this bucket must be
 * emptied by the list".  Two stored objects that carry the same id both take that id's label; ids that no object carries are
 * ignored; *n_named (nullable) <- the OBJECTS (not list entries) that took their label from the list.  One call is a split (name one
 * bucket's objects: lmi_bucket_read gives their ids), a merge (a many-to-one map, n == 0), a new empty bucket between existing ones
 * (an injective map into a larger L_new) or a complete re-placement after retraining (name everything).
 * THE ORDER RULE: *out holds exactly what lmi_create + h's settings + lmi_buckets_begin(.., L_new, new labels ..) / add_rows / end
 * would hold for the object list "h's objects in the order h holds them -- old bucket ascending, then row within the bucket -- each
 * with its new label".  So a new bucket's objects are ordered by (old bucket, old row), whatever the order of the list or the map:
 * every search returns the same dists, ids and keys bit for bit, lmi_bucket_sizes / lmi_bucket_read / lmi_bucket_read_f16 /
 * lmi_index_bytes return the same, and lmi_debug_layout shows a fresh build's layout with all four counters zero.  The identity call
 * (n == 0, NULL map, L_new == L) is h's compaction, equal to lmi_subset(h, NULL, 0, LMI_SUBSET_DROP, ..).  The order is that of the
 * unique words (new label << 32) | ordinal, ordinal = the object's dense position in h's order (NOT its slab row: an insert may have
 * moved a bucket behind later ones); no position depends on the arrival order of an atomic, on the sort's tile length or on a grid.
 * *out is a NEW, INDEPENDENT handle on h's device, as lmi_subset's: no clone view, h may be destroyed first, either may be mutated
 * without the other noticing.  It carries h's settings, storage and chunk rule (lmi_subset's list) and copies of ALL of h's models,
 * but NOT the tree tables (their child_bucket entries name h's buckets): set what changed with lmi_set_mlp / lmi_nav_set_model /
 * lmi_nav_set_tree, which work on a built handle.  lmi_search refuses a root model whose class count is not L_new, as ever; the
 * explicit-order calls (lmi_scan_topk, lmi_scan_union, lmi_scan_range) work at once.  Its layout is its own: a filter of h is refused.
 * All three stored forms: row-major f32 (both metrics; the -|x|^2/2 column of L2 travels with the row), f32 fragments
 * (lmi_set_prefilter(0)) and LMI_STORAGE_F16, whose halves are moved as stored under h's scale (the object set is h's, so the absmax
 * is) -- no binary32 image exists at any point.  The fp16 fragments, norms and bounds are derived from the new handle's own rows.
 * The call synchronises h's stream first, only READS h -- allowed while clone views live, and on one -- and returns when the new
 * index is complete.  Peak device memory: h's images + the new index's + the call's maps: 20 bytes per object of h (two buffers of
 * 8-byte words -- one when a single sort tile holds them all -- and the 4-byte slab row of each ordinal) + 4 bytes per slab row of the
 * new index (the gathers' source positions) + 8 bytes per list entry (its id and its label); the maps are freed before the call
 * returns.
 * Refused before any launch, with *out left NULL and h untouched, each by name: NULL h or out; h not built or being built; L_new < 1
 * or >= 2^20; n < 0, or n > 0 with a NULL ids or labels; a label outside [0, L_new); a map entry outside [-1, L_new); a NULL map with
 * L_new < L; an id listed twice (the message says which); a handle built with an `owned` mask (a new partition needs a new
 * ownership).  Refused after the labelling pass: an object that is not named and whose bucket maps to -1 (the message names the first
 * such bucket and how many of its objects were left); a layout past the 32-bit slab positions; a failed allocation (the message says
 * how many bytes it wanted).  Then no index is made and everything the call allocated is freed. */
LMI_API int lmi_regroup(lmi_index *h, const uint32_t *ids, const int64_t *labels, int64_t n, const int32_t *bucket_map /* nullable */,
                        int L_new, lmi_index **out, int64_t *n_named /* nullable */);
/* Test hook, per thread: the tile length of lmi_regroup's sort (0: the default 8 192; a power of two in [64, 8192]).  Objects up to
 * one tile are sorted in LDS alone; above it tiles are sorted and merge passes double the runs.  Never changes a bit of the result. */
LMI_API int lmi_regroup_set_geometry(int64_t tile_rows);
enum {
    LMI_REGROUP_PLAN_ROWS = 0,     /* objects of the source = words sorted                              */
    LMI_REGROUP_PLAN_TILE_ROWS,    /* T                                                                 */
    LMI_REGROUP_PLAN_TILES,        /* tiles sorted in LDS: ceil(rows / T)                               */
    LMI_REGROUP_PLAN_MERGE_ROWS,   /* words of one merge piece: min(T, 2 048)                           */
    LMI_REGROUP_PLAN_PASSES,       /* merge passes (0: one tile held every word)                        */
    LMI_REGROUP_PLAN_MAP_BYTES,    /* device bytes of the call's maps                                   */
    LMI_REGROUP_PLAN_NAMED,        /* *n_named                                                          */
    LMI_REGROUP_PLAN_COUNT
};
/* What the last lmi_regroup on this thread did (all zero after a refused call): out[0..n) <- the first
 * min(n, LMI_REGROUP_PLAN_COUNT) words. */
LMI_API int lmi_debug_regroup_plan(int64_t *out, int n);
/* Several built indexes over the same partition as ONE new index, derived on the device (no reference counterpart: the reference
 * concatenates its DataFrames and rebuilds).  lmi_subset is "same labels, fewer objects", lmi_regroup "same objects, new labels"; this
 * is "same labels, the objects of parts[0..n_parts)".  It is how an LMI_STORAGE_F16 index, which lmi_buckets_insert refuses, grows
 * (build the delta as a small index, fold it in), how an index is assembled from parts built separately, and how several mutated
 * handles are compacted in one pass.  *n_total (nullable) <- the objects the new index stores.
 * THE ORDER RULE: *out holds exactly what lmi_create + parts[0]'s settings + lmi_buckets_begin / add_rows / end would hold for the
 * object list "parts[0]'s objects in the order it holds them -- bucket ascending, then row within the bucket --, then parts[1]'s, and
 * so on, each with its bucket as its label".  So bucket b of the result is parts[0]'s bucket b, followed by parts[1]'s bucket b, and
 * so on: every search (lmi_search, lmi_scan_topk, the tree walk and, where the stored form allows them, the union and range calls)
 * returns the same dists, ids and keys bit for bit, lmi_bucket_sizes / lmi_bucket_read / lmi_bucket_read_f16 / lmi_index_bytes
 * return the same, and lmi_debug_layout shows a fresh build's layout with all four counters zero.  A single part is therefore that
 * part's compaction, equal to lmi_subset(h, NULL, 0, LMI_SUBSET_DROP, ..).  No position depends on the arrival order of an atomic or
 * on a grid.
 * *out is a NEW, INDEPENDENT handle on the parts' device, as lmi_subset's: no clone view, every part may be destroyed first, any may
 * be mutated without the others noticing.  It carries copies of parts[0]'s models and tree tables -- valid, because L and the
 * buckets' meaning are the same --, parts[0]'s settings and chunk rule (lmi_subset's list) and a layout stamp of its own: a filter
 * made on a part is refused on it.  The other parts' models are ignored.  A part may be listed twice; its objects then appear twice.
 * Ids are the caller's and are not compared across parts, as with lmi_buckets_insert.
 * All three stored forms: row-major f32 (both metrics; rows are moved as stored, the -|x|^2/2 column of L2 travels with its row; the
 * fp16 fragments, absmax, scale, norms and bounds are derived from the new handle's own rows), f32 fragments (lmi_set_prefilter(0))
 * and LMI_STORAGE_F16, whose halves are moved out of the fragments -- no binary32 image exists at any point.  Every F16 part stores
 * x * s_t under its own scale; the result's scale s_out is that of the largest of the parts' maxima (each handle keeps its own: no
 * pass over the rows) and part t's halves are multiplied by the power of two s_out / s_t <= 1 on the way.  Going down in exponent
 * can lose bits: if a half changes when it is rounded back the call is refused with the words lmi_buckets_end has for such data --
 * the verdict a fresh build of the concatenated rows reaches, for which x * s_out must be a half too.
 * Sharded ranks: either every part carries an `owned` mask and the masks are equal, or none does; the result carries the mask, a
 * bucket holds rows on some rank if it does so in any part, and N is the sum of the parts' N.
 * The call synchronises every part's stream first, then only READS the parts -- allowed on clone views and while clone views of a
 * part live -- and returns when the new index is complete.  Peak device memory: the parts' images + the new index's + 8 bytes per
 * slab row of the new index (the source map, freed before the call returns).
 * Refused before any launch, with *out left NULL and every part untouched, each by name: NULL parts or out, a NULL part; n_parts
 * outside [1, LMI_CONCAT_MAX_PARTS]; a part that is not built or is being built; parts on different devices; a part that differs
 * from parts[0] in d, L, the metric, the storage, the prefilter (on / off) or the `owned` mask (the message names the part and the
 * property); a bucket or a layout past the 32-bit slab positions.  Refused after launches: the F16 scale loss above, and a failed
 * allocation (the message says how many bytes it wanted).  Then no index is made and everything the call allocated is freed. */
#define LMI_CONCAT_MAX_PARTS 64
LMI_API int lmi_concat(lmi_index *const *parts, int n_parts, lmi_index **out, int64_t *n_total /* nullable */);
enum {
    LMI_CONCAT_PLAN_PARTS = 0,       /* n_parts                                                           */
    LMI_CONCAT_PLAN_ROWS,            /* objects the new index stores = *n_total                           */
    LMI_CONCAT_PLAN_SLAB_ROWS,       /* rows of the new slab: 32 per row-block of the fresh layout        */
    LMI_CONCAT_PLAN_MAP_BYTES,       /* device bytes of the call's maps                                   */
    LMI_CONCAT_PLAN_RESCALED_PARTS,  /* LMI_STORAGE_F16: parts whose halves were multiplied (ratio < 1)   */
    LMI_CONCAT_PLAN_COUNT
};
/* What the last lmi_concat on this thread did (all zero after a refused call): out[0..n) <- the first
 * min(n, LMI_CONCAT_PLAN_COUNT) words. */
LMI_API int lmi_debug_concat_plan(int64_t *out, int n);
/* sizes[L] <- number of objects per bucket (0 for buckets not owned). */
LMI_API int lmi_bucket_sizes(lmi_index *h, int64_t *sizes);
/* Reads one bucket back to the host in bucket order (what `data_search.loc[g.index].to_numpy()`
 * and `g.index.to_numpy()` return, LearnedIndex.py:351,357): rows[n_b][d], ids[n_b]; either may
 * be NULL. */
LMI_API int lmi_bucket_read(lmi_index *h, int bucket, float *rows, uint32_t *ids);

/* Binary16 rows as they are distributed (no reference counterpart: the reference holds float32 DataFrames).  "Half" is IEEE
 * binary16, passed as its uint16_t bit pattern -- an includer needs no _Float16.  One contract for every *_f16 entry point of this
 * header: the call returns bit for bit what its namesake returns for the same values widened to binary32 (widening is exact).
 * A half pointer need only be 2-byte aligned, on the host and -- with on_device -- on the device: the kernels read 16 bytes at a
 * time only where d % 8 == 0 and the piece's base is 16-byte aligned, element by element otherwise.
 * lmi_buckets_add_rows_f16 / lmi_buckets_add_owned_rows_f16: as lmi_buckets_add_rows / _add_owned_rows (same checks, same piece size
 *        in rows, so half the staging and half the upload).  LMI_STORAGE_F16: the halves go into the fragments as they are -- no
 *        binary32 copy of any piece exists; LMI_STORAGE_F32 (prefilter on or off, either metric): the staged piece is widened on the
 *        device and ingested like a float piece.  Half and float pieces may be mixed freely within one build, piece by piece; the
 *        rule that add_rows and add_owned_rows are not mixed covers all four calls.  lmi_buckets_end's verdict is unchanged (a half
 *        piece can only fail it by inf / NaN or by the scale).
 * lmi_buckets_insert_f16: as lmi_buckets_insert, its checks and refusals included (an LMI_STORAGE_F16 index is refused).
 * lmi_knn_f16 / lmi_knn_range_f16 (declared beside lmi_knn and lmi_knn_range below): the exact ground truths on queries AND base
 *        as halves; the same contract, and the base is never widened into a buffer.
 * lmi_kmeans_f16 / lmi_train_f16 / lmi_mlp_topk_f16 (declared beside their namesakes below): the index build -- clustering, training
 *        and the placement check -- on rows as halves; the same contract. */
LMI_API int lmi_buckets_add_rows_f16(lmi_index *h, const uint16_t *rows, int64_t row0, int64_t nrows, int on_device);
LMI_API int lmi_buckets_add_owned_rows_f16(lmi_index *h, const uint16_t *rows, const int64_t *index, int64_t nrows,
                                   int on_device);
LMI_API int lmi_buckets_insert_f16(lmi_index *h, const uint16_t *rows, const int64_t *labels, const uint32_t *ids, int64_t nrows,
                                   int on_device, int64_t *n_stored);
/* lmi_bucket_read with the rows as halves [n_b][d] (no reference counterpart).  LMI_STORAGE_F16: the halves that were ingested
 * (undoing the index scale and narrowing are exact by the admissibility rule).  LMI_STORAGE_F32, prefilter on or off: narrowed on the
 * device; if any value of the bucket is not finite or not exactly representable in binary16 the call fails, says so, and writes
 * no row -- nothing approximate is ever served, as with lmi_buckets_end.  The index is unchanged either way; the L2 norm column is
 * not returned. */
LMI_API int lmi_bucket_read_f16(lmi_index *h, int bucket, uint16_t *rows, uint32_t *ids);

/* Stored objects by id (the resident counterpart of `data_search.loc[ids]`, LearnedIndex.py:357; lmi_bucket_read needs the bucket
 * number, this call finds it).  For request i:
 *   bucket[i], row[i]   the location of the FIRST live stored row whose id equals ids[i], first in lexicographic order: bucket
 *                       ascending, then row within the bucket ascending -- not slab position (after lmi_buckets_insert / _delete a
 *                       bucket may lie anywhere in the slab).  (-1, -1): no live row carries the id.  Stored ids are the caller's and
 *                       may repeat; the rule holds bit for bit on any grid (the minimum of a set does not depend on the order it is
 *                       taken in).
 *   rows[i][0..d)       exactly what lmi_bucket_read(bucket[i]) (lmi_rows_fetch_f16: lmi_bucket_read_f16) returns at index row[i]:
 *                       the row-major values (LMI_STORAGE_F32, prefilter on), the f32 fragments unpacked (lmi_set_prefilter(0)), the
 *                       halves widened and unscaled, both exact (LMI_STORAGE_F16).  The L2 norm column is not returned.  An absent id
 *                       gets a row of zeros.
 * Request ids need not be sorted and may repeat; every occurrence gets the same answer.  rows, bucket and row are each nullable, at
 * least one must be given; rows == NULL makes the call a pure locate.  on_device covers all four pointers: ids on the device are
 * copied to the host (4n bytes, the one internal synchronisation -- the list is sorted there), and with rows on the device the
 * vectors never leave it.
 * lmi_rows_fetch_f16: the rows as halves.  LMI_STORAGE_F16: the halves that were ingested.  The two f32 forms are narrowed on the
 * device, as by lmi_bucket_read_f16: if any fetched value is not finite or not exactly representable in binary16 the call fails and
 * says so; host outputs (rows, bucket, row) then receive nothing, a device `rows` buffer has unspecified content.  The zero rows of
 * absent ids do not count.
 * How: the ids are sorted and de-duplicated on the host; every live row of the index searches its id in that list (one pass over the
 * ids, 4N bytes) and lowers the id's word of a location table with one 64-bit atomicMin; one gather per piece of requests reads the
 * located rows out of the stored image.  No id table is kept between calls, so a mutation can never make one stale.  Device memory
 * of the call: at most 16n bytes of tables, freed before it returns, and -- for host outputs -- the handle's staging buffer, one
 * piece of requests at a time (what 64 MiB hold; device outputs are written in place, 2^24 requests per launch).  Besides the
 * outputs one more transfer reaches the host, with device pointers too: the location table, 8 bytes per distinct id, ahead of the
 * closing synchronisation -- lmi_debug_fetch_plan's FOUND is counted from it.
 * The call only reads: clone views, lmi_subset / lmi_regroup / lmi_concat results and sharded ranks are served alike (a rank reports
 * the ids of buckets it does not own as absent: those buckets hold no live rows there).  It synchronises the handle's stream before it
 * returns, like lmi_bucket_read.
 * Refused before any launch: a NULL handle; an index that is not built; n < 0 or n >= 2^31; NULL ids with n > 0; rows, bucket and row
 * all NULL.  n == 0 succeeds and writes nothing. */
LMI_API int lmi_rows_fetch(lmi_index *h, const uint32_t *ids, int64_t n, float *rows /* nullable */, int32_t *bucket /* nullable */,
                           int32_t *row /* nullable */, int on_device);
LMI_API int lmi_rows_fetch_f16(lmi_index *h, const uint32_t *ids, int64_t n, uint16_t *rows /* nullable */,
                               int32_t *bucket /* nullable */, int32_t *row /* nullable */, int on_device);
/* Test hook: requests per piece (one gather launch and, for host outputs, one round through the staging buffer) of the fetch calls
 * on this thread, host and device outputs alike; 0 = the default (host outputs: what a 64-MiB stage holds; device outputs: 2^24).
 * Refused outside [0, 2^24].  Never changes a result. */
LMI_API int lmi_fetch_set_geometry(int64_t piece_rows);
enum {
    LMI_FETCH_PLAN_REQUESTS = 0,     /* n                                                                 */
    LMI_FETCH_PLAN_UNIQUE,           /* distinct requested ids                                            */
    LMI_FETCH_PLAN_PIECES,           /* pieces the requests were cut into                                 */
    LMI_FETCH_PLAN_PIECE_ROWS,       /* requests per piece (the last may hold fewer)                      */
    LMI_FETCH_PLAN_FOUND,            /* requests whose id a live row carries (every occurrence counts)    */
    LMI_FETCH_PLAN_FORM,             /* the stored form read: 0 f32 fragments, 1 row-major f32, 2 fp16 fragments */
    LMI_FETCH_PLAN_WORKSPACE_BYTES,  /* device bytes of the call's tables + the stage it asked for        */
    LMI_FETCH_PLAN_COUNT
};
/* What the last lmi_rows_fetch / lmi_rows_fetch_f16 on this thread did (all zero after a refused or failed call; n == 0 reports
 * the form only): out[0..n) <- the first min(n, LMI_FETCH_PLAN_COUNT) words. */
LMI_API int lmi_debug_fetch_plan(int64_t *out, int n);

/* Navigation: bucket_order[nq][nb] <- the nb most probable classes per query, most probable first.
 * logits (nullable) [nq][L] <- raw outputs of the last Linear layer.
 * With on_device, queries_nav (here and in every call that takes it) must be 16-byte aligned -- any whole device allocation is:
 * where the input width is a multiple of 4 the fused kernel reads it 16 bytes at a time.
 * Non-finite values: a logit of -inf is an ordinary value (it ranks last, lower class first, with probability 0).  A NaN logit
 * compares with nothing, so it is never selected: a query's ranks run out after its comparable classes and the remaining ranks
 * are class -1 (in lmi_mlp_proba with probability NaN, and the row sum makes every other probability of that query NaN too; a
 * query whose logits are all NaN -- a NaN feature, for one -- gets -1 and NaN throughout).  The oracle defines no order there;
 * the fused and the per-layer forms return the same bits. */
LMI_API int lmi_mlp_topk(lmi_index *h, const float *queries_nav, int nq, int nb, int32_t *bucket_order,
                 float *logits, int on_device);

/* NeuralNetwork.predict_proba (model.py:226-241): probs[nq][L] = softmax of the outputs sorted
 * descending, classes[nq][L] = the matching class indices (int32; the reference returns int64). */
LMI_API int lmi_mlp_proba(lmi_index *h, const float *queries_nav, int nq, float *probs, int32_t *classes,
                  int on_device);

/* Scan: for every query, top-LMI_K_PER_BUCKET by inner product inside each of its nb buckets,
 * dist = 1 - ip (binary32), merged over the ranks to k results (k <= LMI_MAX_K).
 * dists[nq][kout], ids[nq][kout] with kout = (nb == 1 ? LMI_K_PER_BUCKET : k).
 * Unvisited slots: dist = +inf, id = 0.  keys (nullable) [nq][kout] <- rank*16 + position, the
 * tie-break key needed by lmi_merge_gathered.
 * Non-finite and extreme values: for every input the all-f32 scan accepts, the fp16 prefilter returns the all-f32 scan's ids and
 * distance bits, which are the oracle's -- NaN, +-inf and subnormal values and values whose products overflow included, in stored
 * rows and in queries.  A score that is NaN, -inf or -FLT_MAX is never returned (the oracle's insertion test is `s > worst`, from
 * -FLT_MAX); a +inf score is returned, under the inner product with dist = -inf.  A slot left with fewer than LMI_K_PER_BUCKET
 * admissible rows is padded as a short bucket is (the worst distance of the metric, the bucket's last id), and a special value in
 * one query changes no other query's answer.  (The prefilter serves such a slot from its exact fallback: a bound that is not
 * finite, or under L2 a |q|^2 that is not, sends the slot's whole bucket through the canonical chain.)  Left unspecified: under
 * LMI_METRIC_L2 a query with an infinite component -- its distances are fmaf(-2, +-inf, +inf) = NaN, and no order of NaNs is defined. */
LMI_API int lmi_scan_topk(lmi_index *h, const float *queries_search, int nq, const int32_t *bucket_order,
                  int nb, int k, float *dists, uint32_t *ids, uint32_t *keys, int on_device);

/* lmi_mlp_topk followed by lmi_scan_topk, nothing leaves the device in between. */
LMI_API int lmi_search(lmi_index *h, const float *queries_nav, const float *queries_search, int nq, int nb,
               int k, float *dists, uint32_t *ids, uint32_t *keys, int32_t *bucket_order,
               int on_device);

/* lmi_scan_topk / lmi_search / lmi_search_tree with every query array as halves (no reference counterpart; the contract of
 * lmi_buckets_add_rows_f16 above: the results of the namesake on the widened queries, bit for bit).  Host pointers: the halves are
 * uploaded -- half the bytes -- and widened on the device into the handle's query buffers (lmi_search_tree_f16 uploads the scan
 * vectors beside the walk, like its namesake, and widens them behind the join).  on_device: the halves are widened into the handle's
 * buffers; the caller's memory is only read.  queries_search == queries_nav keeps its meaning: one array.  Everything else --
 * arguments, outputs, settings, timings -- as the namesakes.  lmi_pipeline_submit takes binary32 queries only. */
LMI_API int lmi_scan_topk_f16(lmi_index *h, const uint16_t *queries_search, int nq, const int32_t *bucket_order,
                      int nb, int k, float *dists, uint32_t *ids, uint32_t *keys, int on_device);
LMI_API int lmi_search_f16(lmi_index *h, const uint16_t *queries_nav, const uint16_t *queries_search, int nq, int nb,
                   int k, float *dists, uint32_t *ids, uint32_t *keys, int32_t *bucket_order, int on_device);
LMI_API int lmi_search_tree_f16(lmi_index *h, const uint16_t *queries_nav, const uint16_t *queries_search, int nq, int nb, int k,
                        float *dists, uint32_t *ids, uint32_t *keys, int32_t *slab_ids, int32_t *entries, int on_device);
/* lmi_mlp_topk with queries_nav as halves, by the same front as lmi_search_f16: host halves are uploaded as they are and widened on the
 * device into the handle's buffer, device halves (2-byte aligned; only read) are widened from where they lie.  bucket_order and
 * logits are those of lmi_mlp_topk on the widened queries, bit for bit; refusals as there, naming lmi_mlp_topk_f16.  The placement
 * check of an index build on halves goes through this call.  There is no lmi_mlp_proba_f16. */
LMI_API int lmi_mlp_topk_f16(lmi_index *h, const uint16_t *queries_nav, int nq, int nb, int32_t *bucket_order,
                     float *logits, int on_device);

/* Multi-GPU: gathered_{dists,ids,keys}[w] is rank w's lmi_scan_topk output [nq][kout], found
 * world_stride elements after rank w-1's (0 -> dense, nq*kout; a packed all-gather of
 * [dists|ids|keys] per rank uses 3*nq*kout); writes the merged dists/ids [nq][kout]. */
LMI_API int lmi_merge_gathered(lmi_index *h, const float *gathered_dists, const uint32_t *gathered_ids,
                       const uint32_t *gathered_keys, int world, int64_t world_stride, int nq,
                       int kout, float *dists, uint32_t *ids, int on_device);

/* Copies `bytes` from device memory to any device-accessible destination -- in particular PINNED host memory
 * (hipHostMalloc / torch pin_memory) -- by a kernel on the handle's stream: the result download of a pipelined
 * caller (learnedmetricindex_amd/pipeline.py) without hipMemcpyAsync, whose D2H form was seen to block the
 * submitting host thread for milliseconds behind queued kernels (ROCm 7.2).  Both pointers 16-byte aligned.
 * Replaces the `.cpu().numpy()` of model.py:240-241 / the numpy results of LearnedIndex.py:340-341. */
LMI_API int lmi_copy_out(lmi_index *h, void *dst, const void *src, int64_t bytes);
/* Up to 4 such copies as ONE launch (dists, ids and the bucket order of a batch: three launches were 25 us of a 0.6-ms search). */
LMI_API int lmi_copy_out_many(lmi_index *h, int n, void *const *dst, const void *const *src, const int64_t *bytes);
/* One batch of a host-in -> host-out pipeline as ONE call (learnedmetricindex_amd/pipeline.py: a dozen Python-level stream / event / ctypes
 * operations per batch are 0.2-0.3 ms of host time -- more than the GPU's 0.17 ms for a 1 000-query search).  Streams and events are the caller's
 * (hipStream_t / hipEvent_t as void*): upload of the pinned host queries on s_in -> ev_in; overlap_nav != 0: lmi_mlp_topk on s_nav behind ev_in
 * -> ev_nav, lmi_scan_topk on s_run behind ev_nav; else lmi_search on s_run behind ev_in; (dists, ids) are stored where dists_out / ids_out point
 * (device memory, or pinned host memory: then no download is needed); the bucket order goes to bo_dev and, bo_host != NULL, by one copy
 * kernel to pinned bo_host; ev_out is recorded on s_run behind everything.  qs_host == NULL: navigation and scan vectors are the same array.
 * The handle's stream is s_run on return.  Replaces the body of LearnedIndex.search for one batch (LearnedIndex.py:85-159) like lmi_search. */
LMI_API int lmi_pipeline_submit(lmi_index *h, void *s_in, void *s_nav, void *s_run, void *ev_in, void *ev_nav, void *ev_out,
                                const float *qn_host, const float *qs_host, float *qn_dev, float *qs_dev, int nq, int nb, int k,
                                float *dists_out, uint32_t *ids_out, int32_t *bo_dev, int32_t *bo_host, int overlap_nav);

/* The same exchange through RCCL inside the library (no reference counterpart; SURVEY 8b `lmi_allgather_merge(h,
 * ncclComm_t, ...)`): a C/C++ caller runs the bucket-sharded mode without torch.distributed.
 *   lmi_comm_unique_id   rank 0: 128 bytes (ncclUniqueId) to hand to every rank by any side channel
 *   lmi_comm_init        every rank: *comm <- ncclComm_t over `world` ranks on the handle's device (collective call)
 *   lmi_allgather_merge  every rank: its lmi_scan_topk / lmi_search outputs (DEVICE pointers [nq][kout], keys
 *                        included) -> ONE ncclAllGather of the packed [dists|ids|keys] block on the handle's stream
 *                        -> merge kernel -> dists/ids [nq][kout] (device), identical on every rank.  `comm` may be
 *                        any ncclComm_t of the process (e.g. PyTorch's).
 * RCCL is resolved at run time (the process image, else librccl.so); the calls fail cleanly when it is absent. */
LMI_API int lmi_comm_unique_id(void *id128);
LMI_API int lmi_comm_init(lmi_index *h, int rank, int world, const void *id128, void **comm);
LMI_API int lmi_comm_destroy(void *comm);
LMI_API int lmi_allgather_merge(lmi_index *h, void *comm, int rank, int world, const float *local_dists,
                        const uint32_t *local_ids, const uint32_t *local_keys, int nq, int kout, float *dists,
                        uint32_t *ids);

/* faiss.knn(xq, xb, k, metric=METRIC_INNER_PRODUCT) on host pointers: D[nq][k] similarities in
 * descending order, I[nq][k] row numbers; nb < k pads with D = -FLT_MAX, I = -1.  k <= 10. */
LMI_API int lmi_knn_ip(int device, const float *xq, int64_t nq, const float *xb, int64_t nb, int d, int k,
               float *D, int64_t *I);

/* Lloyd's k-means on the device, deterministic (replaces the label provider of the index build:
 * faiss.Kmeans(d, k, niter=20, seed=2023).train(x); index.search(x, 1)     li/clustering/faiss_kmeans.py:8-24; seeding is the
 * caller's: `centroids` carries the initial centroids in).  The same input gives the same centroids and labels bit for bit on any
 * launch geometry; tests/kmeans_ref.py restates the call in numpy on top of oracle.knn_l2.
 * No handle (like lmi_knn_ip): the work runs on the NULL stream of `device` and the call returns when the outputs have landed.
 * on_device covers x [n][d], centroids [k][d] and labels [n]: device pointers, x is only read; otherwise host pointers -- x is
 * uploaded once, in pieces, and stays resident for all passes.  counts [k] and changed [niter+1] are host pointers, nullable.
 * Arithmetic contract
 *   assignment   cn_j = the chain acc = fmaf(c[t], c[t], acc) from 0, t = 0..d-1; s_ij = the chain acc = fmaf(x[t], c[t], acc)
 *                from 0; key_ij = fmaf(1.0f, -0.5f * cn_j, s_ij) -- the key of LMI_METRIC_L2 (oracle.knn_l2).  label_i starts at 0
 *                with best = key_i0 and becomes j only when key_ij > best, j ascending: ties go to the lower centroid, a NaN never wins.
 *   update       e = the smallest integer with max|x| < 2^e (0 for all-zero data); q(v) = rint(v * 2^(36-e)): the product is exact
 *                in binary64, the rounding is to nearest even, the result an int64.  S = the sum of q(x) over a cluster's rows per
 *                dimension, in int64: |q| <= 2^36 and n <= 2^26, so |S| <= 2^62, and integer addition is associative -- any
 *                reduction tree, grid or atomic order gives the same S.  A cluster with cnt > 0 gets
 *                c = (float)((double)S / (double)cnt * 2^(e-36)): one int64 -> binary64 conversion, one IEEE binary64 division, an
 *                exact scaling, one rounding to binary32.  A cluster with cnt == 0 keeps its centroid.
 *   schedule     pass it = 0..niter assigns; changed[it] = rows whose label differs from the previous pass (labels start at -1:
 *                changed[0] = n); after every pass but the last the centroids are updated.  The labels returned are the assignment
 *                to the centroids returned, counts is their histogram.  A pass it >= 1 with changed[it] == 0 is a fixed point: the
 *                call stops there and the remaining changed entries are 0 -- the result is the same as if it had gone on.
 * Refused, with nothing written: n < 1, d < 1, d > 4096, k < 1, k > n, k > 16384, niter < 0, niter > 1000, n > 2^26 (the bound of
 * the integer sums), NULL x / centroids / labels; and, found on the device in the pass that takes max|x|, any value of x or of the
 * initial centroids that is not finite.  A failed allocation names the bytes it wanted; the call frees all it allocated.
 * Peak device memory: 8n bytes (sorted rows and their labels) + k' * (8d + 4 * roundup(d+1, 32) + 12) with k' = roundup(k, 32) (sums, fragments, counts)
 * + 8 * (niter + 2); with host pointers 4nd + 4kd + 4n more for x, the centroids and the labels. */
LMI_API int lmi_kmeans(int device, const float *x, int64_t n, int d, int k, int niter,
                       float *centroids /* [k][d], in: initial, out: final */, int32_t *labels /* [n] out */,
                       int64_t *counts /* [k] host, nullable */, int64_t *changed /* [niter+1] host, nullable */,
                       int on_device);

/* lmi_kmeans with x [n][d] given as binary16 bit patterns (2-byte alignment is enough, host or device): the index build's clustering
 * on data that is distributed as 16-bit floats, without a widened copy of it on the host or in device memory.  centroids stay binary32,
 * in and out: means are not halves.  The contract is lmi_kmeans's, word for word, on the widened values -- the key, the tie rule, e,
 * q(v), the int64 sums, the division, the schedule, the fixed-point stop: widening a half is exact, so centroids, labels, counts and
 * changed are bit for bit what lmi_kmeans returns on the widened array.  e is that of the widened array too, also where every value
 * is a binary16 subnormal (the maximal half is widened on the host; e comes from the same frexp).
 * Host pointers: x goes up once, as halves, in pieces, and stays resident as halves.  Device pointers: x is read where it is; 16-byte
 * loads are used only where d % 8 == 0 and x is 16-byte aligned, 2-byte loads otherwise.
 * Bounds and refusals: lmi_kmeans's, naming lmi_kmeans_f16; a half that is inf or NaN (bits & 0x7fff >= 0x7c00) is the value that is
 * not finite.  Nothing is written by a refused call.
 * Peak device memory: lmi_kmeans's with 2nd in place of 4nd: 8n + k' * (8d + 4 * roundup(d+1, 32) + 12) with k' = roundup(k, 32)
 * + 8 * (niter + 2); with host pointers 2nd + 4kd + 4n more for x, the centroids and the labels. */
LMI_API int lmi_kmeans_f16(int device, const uint16_t *x, int64_t n, int d, int k, int niter,
                           float *centroids /* [k][d] binary32, in: initial, out: final */, int32_t *labels /* [n] out */,
                           int64_t *counts /* [k] host, nullable */, int64_t *changed /* [niter+1] host, nullable */,
                           int on_device);

/* Adam steps on a Linear/ReLU stack with the cross-entropy loss, on the device, deterministic (replaces the training stage of the
 * index build: NeuralNetwork.train_batch, li/model.py:185-211, whose epoch is ONE optimizer step on its last mini-batch).  The same
 * input gives the same parameters and moments bit for bit on any launch geometry; tests/train_ref.py restates the call in numpy on
 * top of oracle.forward_logits and oracle.softmax.  Initialisation and the choice of rows are the caller's.
 * No handle (like lmi_kmeans): the work runs on the NULL stream of `device` and the call returns when the outputs have landed.
 * on_device covers x [n][dims[0]] and labels [n]: device pointers, only read, the named rows are gathered by a kernel; otherwise host
 * pointers -- only the rows that batch_rows names are gathered on the host and uploaded, in pieces; x itself is never uploaded.
 * Everything else is a host pointer.  W[i] [dims[i+1]][dims[i]] and b[i] [dims[i+1]] in lmi_set_mlp's layout: in the initial, out
 * the trained parameters.  adam [4 * n_layers]: adam[4i .. 4i+3] = m(W_i), v(W_i), m(b_i), v(b_i), in and out; NULL: zeros in, discarded.
 * *t: in the Adam steps taken so far, out += n_steps; NULL: 0.  batch_rows [n_steps][bsz]: the rows of x step s trains on (a row may
 * repeat).  losses [n_steps], nullable.
 * Arithmetic contract -- step s uses the parameters as they stand at its start; B = bsz, rows in batch_rows[s] order
 *   forward      lmi_set_mlp's chain: z_l[r][o] = the chain acc = fmaf(a_l[r][k], W_l[o][k], acc) from b_l[o], k ascending; a_0 = the
 *                rows of x, a_{l+1} = z_l > 0 ? z_l : +0 for every layer but the last.
 *   loss grad.   p = lmi_mlp_proba's softmax of the last z: the maximum by `v > m ? v : m` from class 0, the library's own expf, the
 *                row sum as one chain of adds in class order, one division.  g[r][c] = (p[r][c] - [c == y_r]) * (1.0f / (float)B):
 *                one binary32 subtract, one divide, one multiply.
 *   weight grad. dW_l[o][i] = the chain acc = fmaf(g[r][o], a_l[r][i], acc) from +0, r = 0..B-1.
 *   bias grad.   db_l[o] = the chain acc = acc + g[r][o] from +0, r ascending.
 *   back-prop.   da[r][i] = the chain acc = fmaf(g[r][o], W_l[o][i], acc) from +0, o ascending; then g <- z_{l-1}[r][i] > 0 ? da : +0
 *                (false on NaN).  da_l is taken before W_l is updated.
 *   chains       no chain is split over r, o or k and nothing is added atomically: the result does not depend on the grid.  (The
 *                chains run in v_mfma_f32_32x32x2_f32 and are padded to a multiple of 32 links by fmaf(+0, +0, acc): acc unchanged, -0 -> +0.)
 *   Adam         torch's defaults (betas 0.9 / 0.999, eps 1e-8, no weight decay).  Host, binary64: P1 = 0.9^t', P2 = 0.999^t' as the
 *                t'-fold products of the double literals from 1.0 (no pow), t' = the step's 1-based count; step = (float)(lr / (1 - P1)),
 *                r2 = (float)sqrt(1 - P2).  Per parameter in binary32, every operation rounded on its own:
 *                m = 0.9f*m + 0.1f*grad;  v = 0.999f*v + (0.001f*grad)*grad;  den = sqrtf(v)/r2 + 1e-8f;  param = param - step*(m/den),
 *                sqrtf and / correctly rounded (hipcc's default for binary32; __fsqrt_rn would be the native, unrounded form here).
 *   losses       losses[s] = (float)((1/B) * sum_r -(double)logf(p[r][y_r])), summed in binary64: a diagnostic, not part of the bit
 *                contract (the device's logf is not the host's).
 * Refused, with nothing written: n < 1; n_layers outside 1..LMI_MAX_LAYERS; dims[0] or a hidden width outside 1..4096; classes
 * (dims[n_layers]) outside 1..16384; bsz outside 1..256; n_steps outside 0..100 000; lr not finite or <= 0; *t < 0; a needed pointer
 * NULL; a batch_rows entry outside [0, n); a label of a named row outside [0, classes); and, found on the device before the first
 * step, a named row of x or an initial weight or bias that is not finite.  Parameters that become non-finite during training are
 * not an error.  n_steps == 0 changes nothing.  A failed allocation names the bytes it wanted; the call frees all it allocated.
 * Peak device memory: n_steps * bsz * (4 * dims[0] + 4) for the named rows and their labels (+ 8 * n_steps * bsz with on_device)
 * + the sum over the layers of 12 * out * (in + 1) (parameters and both moments) + 8 * bsz * out (z and g) + 4 * (n_steps + bsz) + 12. */
LMI_API int lmi_train(int device, const float *x, int64_t n, const int32_t *labels /* [n][dims[0]], [n] */,
                      int n_layers, const int *dims, float *const *W, float *const *b /* host; in: initial, out: trained */,
                      float *const *adam /* host, [4*n_layers], in/out; NULL: zeros in, discarded */,
                      int64_t *t /* host; in: steps taken so far, out: += n_steps; NULL: 0 */,
                      const int64_t *batch_rows /* host, [n_steps][bsz] */, int n_steps, int bsz,
                      double lr, float *losses /* host [n_steps], nullable */, int on_device /* covers x and labels */);

/* lmi_train with x [n][dims[0]] given as binary16 bit patterns (2-byte alignment is enough).  The named rows are widened, exactly,
 * into the same binary32 batch buffer lmi_train fills; from there on nothing differs -- same kernels, same finite check, same results,
 * losses included: everything the call returns is bit for bit what lmi_train returns on the widened array.
 * Device pointers: the named rows are gathered and widened by one kernel, label check included.  Host pointers: the named rows are
 * gathered as halves on the host in pieces of the same byte budget (64 MiB), uploaded as halves -- half the bytes -- and widened on
 * the device.  An unnamed row may hold anything; a named row with a half that is inf or NaN is refused by the finite check.
 * Refusals and limits: lmi_train's, naming lmi_train_f16.
 * Peak device memory: lmi_train's; with host pointers + min(64 MiB, 2 * n_steps * bsz * dims[0]) for the piece of halves. */
LMI_API int lmi_train_f16(int device, const uint16_t *x, int64_t n, const int32_t *labels /* [n][dims[0]], [n] */,
                          int n_layers, const int *dims, float *const *W, float *const *b /* host; in: initial, out: trained */,
                          float *const *adam /* host, [4*n_layers], in/out; NULL: zeros in, discarded */,
                          int64_t *t /* host; in: steps taken so far, out: += n_steps; NULL: 0 */,
                          const int64_t *batch_rows /* host, [n_steps][bsz] */, int n_steps, int bsz,
                          double lr, float *losses /* host [n_steps], nullable */, int on_device /* covers x and labels */);

/* Exact brute-force k-NN on the device for k up to LMI_KNN_MAX_K, deterministic (faiss.knn(xq, xb, k, metric) with any k: the
 * ground truth of the reference's Baseline, li/Baseline.py:7-21, and of recall@k).  Its k has nothing to do with the bucket scan's
 * (lmi_knn_ip, k <= 10, stays as it is).  The same input gives the same D and I bit for bit on any launch geometry; oracle.knn_ip
 * and oracle.knn_l2 restate the call.
 * No handle (like lmi_kmeans): the work runs on the NULL stream of `device` and the call returns when D and I have landed.
 * on_device covers xq [nq][d], xb [nb][d], D [nq][k] and I [nq][k]: device pointers, xq and xb are only read and need 4-byte
 * alignment only (xb is read with 16-byte loads where d % 4 == 0 and its base is 16-byte aligned, element by element otherwise;
 * xq always element by element); otherwise host pointers -- xb is uploaded in pieces and each piece is scanned against a group of
 * queries, so the base is never resident as a whole and the device memory of the call does not depend on nb.
 * Arithmetic contract
 *   LMI_METRIC_IP  s = the chain acc = fmaf(q[t], x[t], acc) from +0, t = 0..d-1.  D holds the similarities s, descending.
 *   LMI_METRIC_L2  xn, qn = the same chain on <x,x> and <q,q>; key = the chain s continued by one link fmaf(1.0f, -0.5f * xn, s);
 *                  rows are ranked by key (score = key); D = fmaf(-2.0f, key, qn), ascending.  This is lmi_set_metric's arithmetic.
 *   chains         no chain is split over t.  (The chains run in v_mfma_f32_32x32x2_f32, which keeps subnormals, and are padded to a
 *                  multiple of 32 links by fmaf(+0, +0, acc): acc unchanged, except that a score of -0 -- every link underflowed --
 *                  becomes +0 where d, or d + 1 for L2, is no multiple of 32.)
 *   selection      the first k rows in the total order (score descending, row number ascending; -0 == +0) among the rows whose
 *                  score is > -FLT_MAX: a score that is NaN, -inf or -FLT_MAX is never returned (the oracle's topk_insert from its
 *                  sentinel).  Non-finite inputs are not refused; they do what the chain does with them.
 *   geometry       the order is total and every score is one unsplit chain, so the result does not depend on the tiles, the pieces,
 *                  the splits of a piece, the query groups, the grid or the order in which lists are merged; nothing is added atomically.
 *   padding        fewer than k admissible rows pad with I = -1 and D = -FLT_MAX (L2: FLT_MAX); nb == 0 is all padding; nq == 0
 *                  writes nothing and succeeds.
 * Refused, with nothing written: d outside 1..4096; k outside 1..LMI_KNN_MAX_K; nq or nb < 0 or >= 2^31; an unknown metric; a NULL
 * pointer that is needed (xq, D, I when nq > 0; xb when nq > 0 and nb > 0).  A failed allocation names the bytes it wanted; the call
 * frees all it allocated.
 * Peak device memory, with Q = queries per group (at most 8192 unless forced), Q' = roundup(Q, 32), P = rows per piece (at most
 * 65536 unless forced; with device pointers at most nb), LR = max(256, k rounded up to a power of two), d' = roundup(d, 32) (L2:
 * roundup(d + 1, 32)):  4 Q' roundup(P, 64) (scores) + 8 Q splits LR (lists) + 4 Q' d' (query fragments) + 4 Q + 4 P (norms); with
 * host pointers 4 Q d + 4 P d + 12 Q k more for the queries, the piece and the results.  Q and P shrink when that exceeds 80 % of the
 * free memory.  lmi_debug_knn_plan reports the sum. */
#define LMI_KNN_MAX_K 1024
LMI_API int lmi_knn(int device, const float *xq, int64_t nq, const float *xb, int64_t nb, int d, int k, int metric,
                    float *D /* [nq][k] */, int64_t *I /* [nq][k] */, int on_device);
/* lmi_knn on binary16 inputs: xq [nq][d] and xb [nb][d] are halves (bit patterns), both of them; D and I are typed and laid out as in
 * lmi_knn.  faiss.knn(xq.astype(float32), xb.astype(float32), k, metric) without the widened copies (li/Baseline.py:7-21 on data that is
 * distributed as 16-bit floats).  The contract of every *_f16 entry point (lmi_buckets_add_rows_f16 above): D and I are bit for bit
 * what lmi_knn returns for the same values widened to binary32 -- widening is exact, every half is widened where the kernels load it
 * (the queries into their fragments, the base rows straight into the product's operands) and from there on the arithmetic, the
 * selection and the padding are lmi_knn's; no base row is ever widened into a buffer.
 * Pointers need 2-byte alignment only, on the host and with on_device.  xb is read with 16-byte loads where d % 8 == 0 and the
 * scanned base -- the call's piece buffer with host pointers, the caller's pointer with on_device -- is 16-byte aligned, element by
 * element otherwise (d = 44 is a multiple of 4 and not of 8: element by element); xq always element by element.
 * Host pointers upload halves: 2 Q d + 2 P d instead of 4 Q d + 4 P d in lmi_knn's memory formula; everything else there stands, and
 * the pieces, splits and query groups are the ones lmi_knn makes for the same sizes, forced or not.
 * Refusals and limits: lmi_knn's, with the message naming lmi_knn_f16.  lmi_knn_set_geometry and lmi_debug_knn_plan serve both forms:
 * the plan words are those of the last call of either; VEC_XB reports the 16-byte loads of the form that ran.
 * Not offered: one half array beside a binary32 one; halves in lmi_kmeans / lmi_train. */
LMI_API int lmi_knn_f16(int device, const uint16_t *xq, int64_t nq, const uint16_t *xb, int64_t nb, int d, int k, int metric,
                        float *D /* [nq][k] */, int64_t *I /* [nq][k] */, int on_device);
/* Tuning / test hook: rows of xb per uploaded or scanned piece (< 2^31), base splits per piece (<= 1024; their partial lists are
 * merged afterwards), queries per group (<= 2^20).  0 = chosen by the library.  Thread-local, like lmi_last_error; never changes a
 * result. */
LMI_API int lmi_knn_set_geometry(int64_t piece_rows, int splits, int64_t query_rows);
enum {
    LMI_KNN_PLAN_PIECES = 0,       /* pieces the base was scanned in (0: nb == 0)                                             */
    LMI_KNN_PLAN_PIECE_ROWS,       /* rows per piece (the last may be shorter)                                               */
    LMI_KNN_PLAN_SPLITS,           /* splits per piece = lists per query                                                     */
    LMI_KNN_PLAN_QUERY_GROUPS,     /* groups the queries were taken in                                                       */
    LMI_KNN_PLAN_QUERY_ROWS,       /* queries per group (the last may be smaller)                                            */
    LMI_KNN_PLAN_VEC_XQ,           /* 16-byte loads of xq: always 0, the queries are packed element by element               */
    LMI_KNN_PLAN_VEC_XB,           /* 16-byte loads of xb (lmi_knn_f16: by its own rule, d % 8 == 0)                         */
    LMI_KNN_PLAN_WORKSPACE_BYTES,  /* device bytes the call allocated                                                        */
    LMI_KNN_PLAN_LIST_ROWS,        /* entries of a query's sorted list (LR above)                                            */
    LMI_KNN_PLAN_COUNT
};
/* What the last lmi_knn or lmi_knn_f16 on this thread did (all zero before the first, after a refused call and after one with nq == 0); writes
 * min(n, LMI_KNN_PLAN_COUNT) words. */
LMI_API int lmi_debug_knn_plan(int64_t *out, int n);

/* Exact brute-force RANGE query on the device: for every query ALL rows of xb within distance radius[q] -- the ground truth of the
 * range search (lmi_scan_range below), as lmi_knn is the ground truth of search(k).  It is lmi_knn with another last stage: a
 * threshold and a compaction instead of the selection.  No handle: the work runs on the NULL stream of `device` and the call returns
 * when the result is complete.  on_device covers xq [nq][d] and xb [nb][d], read as lmi_knn reads them (host pointers: xb goes up in
 * pieces and is never resident as a whole); radius is a HOST float [nq], also with on_device.
 * Contract
 *   score        lmi_knn's, word for word.  LMI_METRIC_IP: the chain acc = fmaf(q[t], x[t], acc) from +0, t = 0..d-1.  LMI_METRIC_L2:
 *                xn, qn = the same chain on <x,x> and <q,q>; key = the chain continued by one link fmaf(1.0f, -0.5f * xn, s).  No
 *                chain is split over t and nothing is added atomically (the chains run in v_mfma_f32_32x32x2_f32, padded as in lmi_knn).
 *   distance     IP 1.0f - s; L2 fmaf(-2.0f, key, qn): what lmi_knn writes in D for L2 and what lmi_scan_range writes for IP.
 *   admission    a row is admitted iff its score is > -FLT_MAX (NaN never passes) AND its distance is <= radius[q], compared in
 *                binary32: lmi_scan_range's rule without a filter.  A NaN or -inf radius admits nothing; +inf admits every row that
 *                passes the first rule.
 *   result       an lmi_range_result on `device` (lmi_scan_range below states the object): lims int64 [nq + 1]; dists float; ids
 *                uint32 = the row's number in xb; every query's results in ASCENDING ROW order.  Its nb is 1 and its pair counts are
 *                [nq][1], the per-query totals, so lmi_range_result_total, _lims, _read, _pair_counts, _sort and _destroy work on it
 *                as on any other.  The same bit for bit for any pieces, splits, query groups, grid or pointer kind.
 *   geometry     lmi_knn_set_geometry applies: piece_rows and query_rows as in lmi_knn; splits = the stretches of a piece that
 *                separate waves count and emit.  It never changes a bit.
 * max_total: as in lmi_scan_range -- the most results the whole call may produce; 0 = only memory limits it.  The running count is
 * tested after every piece; when it passes max_total the call fails, says how many results had been counted when it stopped,
 * launches nothing further and produces no result object (*result = NULL).  The next call works.
 * Every (query, row) pair is multiplied once: a piece's scores stay in the slab while they are counted and then emitted.  The counts
 * of every (group, piece) come back to the host to size its chunk exactly: the call synchronises ONCE PER PIECE of every query group,
 * and once behind the final gather.
 * Refused with nothing launched and *result = NULL: d outside 1..4096; nq or nb < 0 or >= 2^31; an unknown metric; a NULL result
 * pointer; a NULL radius or xq with nq > 0; a NULL xb with nq > 0 and nb > 0; a negative max_total.  nq == 0 succeeds with an empty
 * result (lims = {0}); nb == 0 with lims all 0.  A failure at any point frees all the call allocated and leaves *result = NULL.
 * Device memory of a call, with Q, Q', P, d' as in lmi_knn: 4 Q' roundup(P, 64) (scores) + 4 Q' d' (query fragments) + 4 Q + 4 P
 * (norms) + 4 nq (radii) + 12 Q splits (counts and offsets) + 20 per non-empty (query, piece) run (the gather); with host pointers
 * 4 Q d + 4 P d more for the queries and the piece; no lists.  The results twice while the call runs -- 8 bytes per result in
 * exact-size per-piece chunks, 8 per result in the final arrays, allocated once behind the last group -- and once afterwards. */
struct lmi_range_result;
LMI_API int lmi_knn_range(int device, const float *xq, int64_t nq, const float *xb, int64_t nb, int d, int metric,
                          const float *radius /* HOST [nq], also with on_device */, int64_t max_total,
                          struct lmi_range_result **result, int on_device);
/* lmi_knn_range on binary16 inputs: xq and xb are halves (bit patterns), both of them; radius stays a HOST float [nq].  What
 * lmi_knn_f16 is to lmi_knn: the range ground truth of data distributed as 16-bit floats without a widened copy of it (the reference
 * has no range query; lmi_knn_range's place is taken).  The contract of every *_f16 entry point: the result -- lims, dists, ids, pair
 * counts -- is bit for bit lmi_knn_range's for the same values widened to binary32, and it is the same lmi_range_result, so _read,
 * _sort, _pair_counts and _destroy work on it unchanged.  Alignment, the 16-byte rule, the upload (halves) and the geometry as in
 * lmi_knn_f16; max_total, the refusals and the limits as in lmi_knn_range, with the message naming lmi_knn_range_f16.
 * lmi_debug_knn_range_plan reports the last call of either form. */
LMI_API int lmi_knn_range_f16(int device, const uint16_t *xq, int64_t nq, const uint16_t *xb, int64_t nb, int d, int metric,
                              const float *radius /* HOST [nq], also with on_device */, int64_t max_total,
                              struct lmi_range_result **result, int on_device);
enum {
    LMI_KNN_RANGE_PLAN_PIECES = 0,       /* pieces the base was scanned in (0: nb == 0)                                        */
    LMI_KNN_RANGE_PLAN_PIECE_ROWS,       /* rows per piece (the last may be shorter)                                          */
    LMI_KNN_RANGE_PLAN_SPLITS,           /* stretches per piece, each counted and emitted by a wave of its own                */
    LMI_KNN_RANGE_PLAN_QUERY_GROUPS,     /* groups the queries were taken in                                                  */
    LMI_KNN_RANGE_PLAN_QUERY_ROWS,       /* queries per group (the last may be smaller)                                       */
    LMI_KNN_RANGE_PLAN_RESULTS,          /* results of the call: lims[nq]                                                     */
    LMI_KNN_RANGE_PLAN_CHUNK_BYTES,      /* bytes of the per-piece result chunks, all together (8 per result)                 */
    LMI_KNN_RANGE_PLAN_WORKSPACE_BYTES,  /* device bytes the call allocated beside the chunks and the result                  */
    LMI_KNN_RANGE_PLAN_COUNT
};
/* What the last lmi_knn_range or lmi_knn_range_f16 on this thread did (all zero before the first, after a refused or failed call and after one with
 * nq == 0); writes min(n, LMI_KNN_RANGE_PLAN_COUNT) words. */
LMI_API int lmi_debug_knn_range_plan(int64_t *out, int n);

/* The union scan: for every query the k best objects of the UNION of its visited buckets, k up to LMI_UNION_MAX_K -- what any
 * inverted-file index answers to search(k).  (lmi_scan_topk keeps the reference's semantics: at most LMI_K_PER_BUCKET per bucket,
 * merged by rank, k <= LMI_MAX_K; nothing about it changes.)  oracle.knn_ip / oracle.knn_l2 of a query against the concatenated
 * rows of its buckets restate the call (IP: D -> 1 - D; I -> the id at that ordinal; -1 -> padding).
 * Outputs: dists [nq][k], ids [nq][k], counts [nq] (nullable); always k columns, also for nb == 1.  on_device as in lmi_search:
 * every array a device pointer, or every array a host pointer.  The call synchronises the handle's stream internally -- the bucket
 * order comes back to the host, which plans the work per bucket -- and returns when the outputs have landed, also with on_device.
 * Contract
 *   candidates   of query q: the concatenation, over the ranks t = 0..nb-1 with b = bucket_order[q][t] >= 0, of rows 0..n(b)-1 of
 *                bucket b in the order lmi_bucket_read returns them.  A candidate's ordinal is its position in that concatenation.
 *                A rank of -1 (or of no bucket id) contributes nothing; a bucket listed twice contributes twice; a bucket this
 *                handle does not own has no rows.  n(b) is the live count (after lmi_buckets_insert / _delete).
 *   score        the index's canonical chain over the stored width, lmi_scan_topk's arithmetic: IP acc = fmaf(q[t], x[t], acc) from
 *                +0; L2 the same chain on [q, 1] and [x, -|x|^2/2] (the stored column).  No chain is split; nothing is added
 *                atomically.  (The chains run in v_mfma_f32_32x32x2_f32, padded with fmaf(+0, +0, acc) as in lmi_knn.)
 *   selection    the first k candidates in the total order (score descending with -0 == +0, then ordinal ascending) among the
 *                scores > -FLT_MAX: NaN, -inf and -FLT_MAX are never returned (lmi_knn's rule).
 *   output       dist = what the scan writes for that score: IP 1.0f - s, L2 fmaf(-2, key, |q|^2); id = the stored id;
 *                counts[q] = the number of real results; the slots behind them hold dist = +inf, id = 0.
 *   geometry     every (query, rank) is scored against its whole bucket and owns one sorted list; a query's lists are merged in the
 *                total order.  The result does not depend on query groups, waves, tiles or the grid; lmi_union_set_geometry never
 *                changes a bit.
 * The stops (lmi_set_stop_mass, lmi_set_path_mass, lmi_set_stop_rows) act through the bucket order exactly as in lmi_search /
 * lmi_search_tree; lmi_scan_union takes the caller's order as given.
 * Refused before any launch: an index that is not built; k outside 1..LMI_UNION_MAX_K; nb < 1, nb > 1024 or nq * nb >= 2^31;
 * nb * (largest bucket) >= 2^32 - 1 (ordinals are 32-bit); a needed pointer that is NULL; an index whose stored form is not the
 * row-major one (lmi_set_prefilter(0) or LMI_STORAGE_F16: reading candidates out of fragments is left to a follow-up).  nq == 0
 * writes nothing and succeeds.  Clone views and lmi_subset copies are allowed: the call only reads the index.  There is no _f16
 * query form and no lmi_pipeline_submit form; a sharded rank returns its own part (across ranks: lmi_scan_union_part below).
 * What lmi_timings, lmi_scan_stats, lmi_prefilter_stats, lmi_debug_last_plan and lmi_debug_last_mlp_plan report after a union call
 * is not defined; a following ordinary search behaves as if the union call had not happened.
 * Device memory of a call (allocated and freed by it), with Q = queries per group, LR = max(128, k rounded up to a power of two),
 * d' = the stored width rounded up to 32:  a wave's score slab, 4 bytes per (slot, row of its bucket, rounded up to 64) pair, at most
 * 2 GiB unless forced or one tile of 32 slots needs more + 8 Q nb LR (lists) + 4 d' per packed query of a wave (at most 256 MiB) +
 * about 50 bytes per slot of a group (tables); with host pointers 8 Q k + 4 Q more (lmi_scan_union_part: 20 Q k + 4 Q, the staged
 * part; the geometry is still chosen with 8 Q k).  Q is at most what keeps the lists within
 * 1 GiB (at least 32); the slab, then Q shrink when the sum exceeds 80 % of the free memory. */
#define LMI_UNION_MAX_K 1024
LMI_API int lmi_scan_union(lmi_index *h, const float *queries_search, int nq, const int32_t *bucket_order, int nb, int k,
                           float *dists, uint32_t *ids, int32_t *counts, int on_device);
/* lmi_mlp_topk followed by lmi_scan_union; bucket_order (nullable) [nq][nb] <- the order that was scanned. */
LMI_API int lmi_search_union(lmi_index *h, const float *queries_nav, const float *queries_search, int nq, int nb, int k,
                             float *dists, uint32_t *ids, int32_t *counts, int32_t *bucket_order, int on_device);
/* lmi_nav_order followed by lmi_scan_union; slab_ids, entries (nullable) [nq][nb] as lmi_search_tree returns them. */
LMI_API int lmi_search_tree_union(lmi_index *h, const float *queries_nav, const float *queries_search, int nq, int nb, int k,
                                  float *dists, uint32_t *ids, int32_t *counts, int32_t *slab_ids, int32_t *entries, int on_device);
/* Tuning / test hook: queries per group (<= 2^20) and the bytes of a wave's score slab (one tile of 32 slots is taken even where it
 * needs more).  0 = chosen by the library.  Thread-local, like lmi_last_error; never changes a result. */
LMI_API int lmi_union_set_geometry(int64_t query_rows, int64_t slab_bytes);
enum {
    LMI_UNION_PLAN_GROUPS = 0,        /* groups the queries were taken in                                                     */
    LMI_UNION_PLAN_QUERY_ROWS,        /* queries per group (the last may be smaller)                                          */
    LMI_UNION_PLAN_WAVES,             /* waves of the last group (0: none of its slots had rows)                              */
    LMI_UNION_PLAN_SLAB_BYTES,        /* bytes of the score slab (the largest wave's)                                         */
    LMI_UNION_PLAN_LIST_ROWS,         /* entries of a sorted list (LR above)                                                  */
    LMI_UNION_PLAN_LISTS_PER_QUERY,   /* lists per query = nb: one per (query, rank)                                          */
    LMI_UNION_PLAN_WORKSPACE_BYTES,   /* device bytes the call allocated                                                      */
    LMI_UNION_PLAN_VEC_ROWS,          /* 16-byte loads of the index's rows (stored width % 4 == 0)                            */
    LMI_UNION_PLAN_COUNT
};
/* What the last union call on this thread did (all zero before the first, after a refused call and after one with nq == 0); writes
 * min(n, LMI_UNION_PLAN_COUNT) words. */
LMI_API int lmi_debug_union_plan(int64_t *out, int n);

/* The filtered union scan (no reference counterpart): the union scan with every query's candidates restricted to a set of ids -- a
 * tenant, a category, "not these" -- without a second index (lmi_subset makes one; a filter set is one bit per (filter, stored row)).
 * A FILTER SET holds nf filters over one built index.  Filter j is an id list plus a mode: LMI_FILTER_KEEP -- a stored row is ALLOWED
 * iff its id is in the list; LMI_FILTER_DROP -- iff it is not.  The library sorts and de-duplicates the lists; ids the index does not
 * hold are ignored; rows that share an id all follow it; an empty KEEP list allows nothing, an empty DROP list everything.
 * Query q uses filter filter_of[q], an int32 ON THE HOST (also with on_device) in [-1, nf): -1 = unfiltered; a NULL filter_of = every
 * query uses filter 0.
 * Contract: lmi_scan_union's, with the candidate set reduced to the allowed rows.  Ordinals stay the positions in the UNFILTERED
 * concatenation, scores the unsplit canonical chains; selection takes the first k ALLOWED candidates in (score descending with
 * -0 == +0, ordinal ascending) among the scores > -FLT_MAX; dist, id, padding and counts as there.  Restated twice:
 *   oracle.knn_ip / knn_l2 of the query against the concatenation of its buckets' allowed rows;
 *   for a batch that uses one filter: lmi_subset(h, list, mode) followed by lmi_scan_union with the same order, bit for bit.
 * The filter acts on the SCAN, not on the routing: lmi_set_stop_rows, lmi_set_stop_mass and lmi_set_path_mass count live bucket
 * sizes and model probabilities exactly as before -- a bucket whose rows are all disallowed still uses up the budget.
 * A (query, rank) whose (filter, bucket) pair allows no row is neither scored nor selected (lmi_debug_filter_plan counts them).
 * Validity: the masks are keyed by slab position.  A filter set fits the handle it was made from and that handle's clone views, until
 * the layout changes: after lmi_buckets_insert / lmi_buckets_delete, on lmi_subset's output and on any other index it is refused --
 * the message says "stale" -- and must be made again.  It may outlive the handle; it holds nf * (rows / 8, per row-block of 32) bytes
 * of device memory.
 * lmi_filter_create: all pointers are HOST pointers; ids holds the lists back to back, filter j's at [offsets[j], offsets[j + 1]).
 * Refused: a NULL handle or out; an index that is not built; nf outside 1..LMI_FILTER_MAX; offsets[0] != 0, offsets that are not
 * non-decreasing, 2^31 ids or more in all; a mode other than KEEP / DROP; an index of more than 65535 buckets.
 * lmi_filter_counts: out [nf][L] <- the allowed rows per (filter, bucket).  lmi_filter_bucket_mask: out [n_b] <- one byte (0 / 1) per
 * row of the bucket, in lmi_bucket_read's order (for tests and diagnostics).
 * The filtered calls take their parent's arguments plus (f, filter_of).  Refused before any launch: everything the parent refuses
 * (an index that is not stored row-major included); a NULL filter; a stale or foreign filter; a filter_of entry outside [-1, nf).
 * Not offered: filters on lmi_search's rank merge, a filtered lmi_scan_union_part, _f16 query forms, lmi_pipeline_submit. */
typedef struct lmi_filter lmi_filter;
#define LMI_FILTER_KEEP 0   /* the list names the allowed ids    */
#define LMI_FILTER_DROP 1   /* the list names the disallowed ids */
#define LMI_FILTER_MAX 1024 /* filters of one set                */
LMI_API int lmi_filter_create(lmi_index *h, const uint32_t *ids, const int64_t *offsets /* [nf + 1] */, int nf,
                              const int32_t *modes /* [nf] */, lmi_filter **out);
LMI_API int lmi_filter_destroy(lmi_filter *f);
LMI_API int lmi_filter_counts(lmi_filter *f, int64_t *out /* [nf][L] */);
LMI_API int lmi_filter_bucket_mask(lmi_filter *f, int j, int bucket, uint8_t *out /* [n_b] */);
LMI_API int lmi_scan_union_filtered(lmi_index *h, const float *queries_search, int nq, const int32_t *bucket_order, int nb, int k,
                                    float *dists, uint32_t *ids, int32_t *counts, int on_device, const lmi_filter *f,
                                    const int32_t *filter_of /* host [nq], nullable */);
LMI_API int lmi_search_union_filtered(lmi_index *h, const float *queries_nav, const float *queries_search, int nq, int nb, int k,
                                      float *dists, uint32_t *ids, int32_t *counts, int32_t *bucket_order, int on_device,
                                      const lmi_filter *f, const int32_t *filter_of /* host [nq], nullable */);
LMI_API int lmi_search_tree_union_filtered(lmi_index *h, const float *queries_nav, const float *queries_search, int nq, int nb, int k,
                                           float *dists, uint32_t *ids, int32_t *counts, int32_t *slab_ids, int32_t *entries,
                                           int on_device, const lmi_filter *f, const int32_t *filter_of /* host [nq], nullable */);
enum {
    LMI_FILTER_PLAN_FILTERS = 0,      /* filters of the set the call was given                                                */
    LMI_FILTER_PLAN_MASK_BYTES,       /* bytes of the set's masks on the device                                               */
    LMI_FILTER_PLAN_SLOTS,            /* (query, rank) slots of the last group that were scored and selected                  */
    LMI_FILTER_PLAN_SKIPPED,          /* slots of the whole call left out because their (filter, bucket) pair allows no row   */
    LMI_FILTER_PLAN_COUNT
};
/* What the last filtered union call on this thread did (all zero before the first, after a refused call, after one with nq == 0
 * and after an unfiltered union call); writes min(n, LMI_FILTER_PLAN_COUNT) words.  lmi_debug_union_plan reports the same call's
 * geometry. */
LMI_API int lmi_debug_filter_plan(int64_t *out, int n);

/* The range search (no reference counterpart): for every query ALL objects of its visited buckets within distance radius[q] -- the
 * second standard query of a metric index; the length of a query's result is decided by the data, not by a k.  It is the union scan
 * with another last stage: a threshold and a compaction instead of a selection.  tests/range_ref.py restates it in numpy.
 * Contract
 *   candidates, ordinals, scores   lmi_scan_union's, word for word: the concatenation of the rows of the query's ranks in
 *                lmi_bucket_read's order; a rank of -1 contributes nothing, a bucket listed twice contributes twice; the row counts
 *                are the live ones; the score is the unsplit canonical chain (L2: the stored -|x|^2/2 column inside it).
 *   admission    a candidate is admitted iff its score is > -FLT_MAX (the union scan's rule: NaN never passes) AND
 *                sim_to_dist(score) <= radius[q], compared in binary32, where sim_to_dist is the distance the scan writes:
 *                IP 1.0f - s, L2 fmaf(-2, key, |q|^2).  radius is a HOST float [nq], also with on_device.  A NaN or -inf radius
 *                admits nothing; +inf admits every candidate that passes the first rule.
 *   filter       f (nullable; filter_of nullable, HOST int32 [nq], as in lmi_scan_union_filtered): only the rows query q's filter
 *                allows are candidates; ordinals stay the unfiltered ones.  A filter_of without f is refused.
 *   result       a query's admitted candidates in ASCENDING ORDINAL order (by rank, then by row): no sort, and the order is total.
 *                lims int64 [nq + 1] with lims[0] = 0; dists float [lims[nq]]; ids uint32 [lims[nq]]; query q owns
 *                [lims[q], lims[q + 1]).  The same bit for bit for any query grouping, wave cut, grid or pointer kind;
 *                lmi_union_set_geometry applies to these calls and never changes a bit.
 * The stops (lmi_set_stop_mass, lmi_set_path_mass, lmi_set_stop_rows) act through the bucket order exactly as in the union forms:
 * lmi_search_range routes as lmi_search_union does, lmi_search_tree_range as lmi_search_tree_union; lmi_scan_range takes the caller's
 * order as given.  on_device: queries (and the order arrays) are all device pointers or all host pointers.
 * The result is an opaque lmi_range_result that owns the device arrays and the host lims.  It holds no pointer to its handle and may
 * outlive it.  lmi_range_result_total: lims[nq].  _lims: lims [nq + 1] <- the limits.  _read: dists, ids [total] <- the arrays (device
 * pointers with on_device, else host; both may be NULL where total is 0).  _destroy: frees it (NULL: nothing).
 * max_total: the most results the whole call may produce; 0 = only memory limits it.  When the running count passes max_total the
 * call fails, says how many results had been counted when it stopped, launches nothing further and produces no result object
 * (*result = NULL); the handle stays usable.
 * Every (query, bucket) pair is multiplied once: the scores of a wave stay in its slab while they are counted and then emitted.  The
 * counts of every wave come back to the host to size the wave's chunk exactly: the call synchronises the handle's stream ONCE PER
 * WAVE (and once per query group, and once behind the final gather), and returns when the result is complete.
 * Device memory of a call: the union scan's slab, packed queries and tables (no lists) + 28 bytes per slot of a group + 20 per slot
 * of the call (the gather) + 4 nq; the results twice while the call runs -- 8 bytes per result in exact-size per-wave chunks, 8 per
 * result in the final arrays, allocated once behind the last group -- and once afterwards.
 * Refused before any launch: everything lmi_scan_union refuses apart from k -- an index that is not built; nb < 1, nb > 1024,
 * nq * nb >= 2^31; nb * (largest bucket) >= 2^32 - 1; an index that is not stored row-major (lmi_set_prefilter(0), LMI_STORAGE_F16);
 * a needed pointer that is NULL -- everything the filtered forms refuse of a filter (stale, foreign, filter_of outside [-1, nf)); a
 * NULL radius; a NULL result pointer; a negative max_total.  nq == 0 succeeds with an empty result (lims = {0}).
 * Not offered: _f16 query forms, lmi_pipeline_submit.  Nearest first: lmi_range_result_sort below.  Sharded ranks:
 * lmi_join_range_parts below. */
typedef struct lmi_range_result lmi_range_result;
LMI_API int lmi_scan_range(lmi_index *h, const float *queries_search, int nq, const int32_t *bucket_order, int nb,
                           const float *radius /* host [nq] */, const lmi_filter *f /* nullable */,
                           const int32_t *filter_of /* host [nq], nullable */, int64_t max_total, lmi_range_result **result,
                           int on_device);
/* lmi_mlp_topk followed by lmi_scan_range; bucket_order (nullable) [nq][nb] <- the order that was scanned. */
LMI_API int lmi_search_range(lmi_index *h, const float *queries_nav, const float *queries_search, int nq, int nb,
                             const float *radius /* host [nq] */, const lmi_filter *f /* nullable */,
                             const int32_t *filter_of /* host [nq], nullable */, int64_t max_total, lmi_range_result **result,
                             int32_t *bucket_order /* nullable */, int on_device);
/* lmi_nav_order followed by lmi_scan_range; slab_ids, entries (nullable) [nq][nb] as lmi_search_tree returns them. */
LMI_API int lmi_search_tree_range(lmi_index *h, const float *queries_nav, const float *queries_search, int nq, int nb,
                                  const float *radius /* host [nq] */, const lmi_filter *f /* nullable */,
                                  const int32_t *filter_of /* host [nq], nullable */, int64_t max_total, lmi_range_result **result,
                                  int32_t *slab_ids /* nullable */, int32_t *entries /* nullable */, int on_device);
LMI_API int lmi_range_result_total(const lmi_range_result *r, int64_t *total);
LMI_API int lmi_range_result_lims(const lmi_range_result *r, int64_t *lims /* [nq + 1] */);
LMI_API int lmi_range_result_read(const lmi_range_result *r, float *dists, uint32_t *ids, int on_device);
/* The counts behind lims: *nb (nullable) <- the nb of the call that made the result; counts (nullable, HOST int32 [nq][nb]) <- the
 * results of every (query, rank t of the bucket in the query's order) -- 0 for a rank of -1, an empty bucket, one the filter emptied or
 * one the handle does not own.  Row q sums to lims[q + 1] - lims[q].  A result of nq == 0 reports its call's nb and no counts. */
LMI_API int lmi_range_result_pair_counts(const lmi_range_result *r, int32_t *nb /* nullable */,
                                         int32_t *counts /* [nq][nb], nullable */);
LMI_API int lmi_range_result_destroy(lmi_range_result *r);
enum {
    LMI_RANGE_PLAN_GROUPS = 0,        /* groups the queries were taken in                                                     */
    LMI_RANGE_PLAN_QUERY_ROWS,        /* queries per group (the last may be smaller)                                          */
    LMI_RANGE_PLAN_WAVES,             /* waves of the last group (0: none of its slots had rows)                              */
    LMI_RANGE_PLAN_SLAB_BYTES,        /* bytes of the score slab (the largest wave's)                                         */
    LMI_RANGE_PLAN_RESULTS,           /* results of the call: lims[nq]                                                        */
    LMI_RANGE_PLAN_CHUNK_BYTES,       /* bytes of the per-wave result chunks, all together (8 per result)                     */
    LMI_RANGE_PLAN_WORKSPACE_BYTES,   /* device bytes the call allocated beside the chunks and the result                     */
    LMI_RANGE_PLAN_COUNT
};
/* What the last range call on this thread did (all zero before the first, after a refused or failed call and after one with
 * nq == 0); writes min(n, LMI_RANGE_PLAN_COUNT) words. */
LMI_API int lmi_debug_range_plan(int64_t *out, int n);

/* The union scan across the ranks of a bucket-sharded index (no reference counterpart): every rank scans the buckets it owns and
 * hands on a PART; the merge of the parts is what lmi_scan_union returns on one handle that holds the whole index, bit for bit, for
 * any assignment of the buckets (each owned by exactly one part) and any world size.
 * A part is int32 words [LMI_UNION_PART_PLANES][nq][k]; per (query, j < k), best first:
 *   LMI_UPART_SCORE  the bits of the score the selection ordered by (IP: the similarity; L2: the key of the augmented chain)
 *   LMI_UPART_DIST   the bits lmi_scan_union writes in dists
 *   LMI_UPART_ID     the stored id
 *   LMI_UPART_RANK   the position t in bucket_order[q] of the bucket the object came from
 *   LMI_UPART_ROW    its row in that bucket, in lmi_bucket_read's order
 * and behind the real results the padding: SCORE = the bits of -FLT_MAX, DIST = +inf, ID = 0, RANK = ROW = 0xffffffff.
 * Why these planes: the ranks' lists must be merged in the single handle's order, (score, ordinal).  The distance cannot replace the
 * score -- 1.0f - s and fmaf(-2, key, |q|^2) round, two scores may share a distance's bits, and a merge by distance would then order
 * them by key instead of by score.  The ordinal cannot be computed by a rank, which holds its own buckets' counts only (why
 * lmi_set_stop_rows is refused on an `owned` mask); (RANK, ROW) orders exactly as the ordinal does and needs no other rank's counts.
 *
 * lmi_scan_union_part is lmi_scan_union in every respect -- candidates, score, selection, refusals, geometry and its hooks, the plan
 * words, memory (with host pointers the staged part: above) -- except that it writes `part` instead of dists / ids; counts as there.
 * On a handle that owns every bucket the DIST and ID planes and counts equal lmi_scan_union's outputs bit for bit. */
#define LMI_UNION_PART_PLANES 5
enum { LMI_UPART_SCORE = 0, LMI_UPART_DIST, LMI_UPART_ID, LMI_UPART_RANK, LMI_UPART_ROW };
LMI_API int lmi_scan_union_part(lmi_index *h, const float *queries_search, int nq, const int32_t *bucket_order, int nb, int k,
                                int32_t *part /* [5][nq][k] */, int32_t *counts /* [nq], nullable */, int on_device);
/* parts [world][LMI_UNION_PART_PLANES][nq][k], dense: part w as rank w wrote it (an all-gather of the parts is this layout).  Per
 * query the first k of its world * k entries in the total order: score descending (binary32 compare, -0 == +0), then RANK ascending,
 * then ROW ascending, then the lower part index; an entry whose ROW is 0xffffffff is padding and is never selected.  dists / ids
 * [nq][k] <- DIST / ID of the selected entries, +inf / 0 behind them; counts[q] (nullable) <- the number of real entries.  world == 1
 * reproduces the part.  on_device as in lmi_merge_gathered: device pointers -> asynchronous on the handle's stream; host pointers ->
 * the parts are uploaded and the result is copied back before the call returns.  The handle needs no built index: it provides the
 * device and the stream.  One wave per query merges the parts' lists in LDS (32 bytes per entry of LR = max(128, k rounded up to a
 * power of two): at most 32 KiB); no device memory is allocated with device pointers.
 * Refused before any launch: a NULL handle; world outside 1..64; k outside 1..LMI_UNION_MAX_K; nq < 0; a block of 2^31 words or
 * more (world * LMI_UNION_PART_PLANES * nq * k, checked in 64 bits); a needed pointer that is NULL.  nq == 0 writes nothing and
 * succeeds. */
LMI_API int lmi_merge_union_parts(lmi_index *h, const int32_t *parts /* [world][5][nq][k], dense */, int world, int nq, int k,
                                  float *dists, uint32_t *ids, int32_t *counts /* nullable */, int on_device);
/* The same exchange through RCCL inside the library, as lmi_allgather_merge: every rank passes its part (a DEVICE pointer) -> ONE
 * ncclAllGather of the 5 * nq * k words (20 nq k bytes per rank) on the handle's stream -> the merge kernel -> dists / ids / counts
 * (device), identical on every rank.  Refusals as lmi_merge_union_parts, and a NULL communicator or a rank outside 0..world-1; fails
 * cleanly when RCCL is absent. */
LMI_API int lmi_allgather_merge_union(lmi_index *h, void *comm, int rank, int world, const int32_t *part /* device */, int nq, int k,
                                      float *dists, uint32_t *ids, int32_t *counts /* nullable */);

/* The range search across the ranks of a bucket-sharded index (no reference counterpart): every rank calls lmi_scan_range on its
 * handle (built with an `owned` mask: an unowned bucket has no rows there, so the rank answers for exactly the buckets it owns) with
 * the SAME queries, bucket order and radius, and hands on its result as a PART: its pair counts (lmi_range_result_pair_counts) and
 * its dists / ids (lmi_range_result_read).  The join of the parts is what lmi_scan_range returns on one handle that holds all the
 * buckets, bit for bit, for any assignment of the buckets (each owned by exactly one part) and any world size.
 * Why a gather suffices: a range result is in (query, rank t, row) order; every (query, t) names one bucket and one part owns it, so
 * the run of (query, t) comes whole from its owner and no ordering by score is needed (unlike lmi_merge_union_parts).
 * Contract
 *   counts       HOST int32 [world][nq][nb], always: counts[r][q][t] = results of part r for (q, t).
 *   dists, ids   [world] pointers: part r's arrays in (q, t, row) order as lmi_range_result_read gives them, counts[r] summed long.
 *                on_device: all device pointers, or all host pointers -- a host part's arrays are uploaded once each.  A part whose
 *                total is 0 may pass NULL for both.
 *   result       the run of (q, t) is the run of the one part whose counts[r][q][t] > 0, copied unchanged, at the exclusive sum of
 *                the summed counts in (q, t) order; lims[q] = that sum at (q, 0).  The result's pair counts are the sum over the
 *                parts.  It is an lmi_range_result like any other (device arrays, host lims; it may outlive the handle) and is
 *                complete when the call returns (the handle's stream is synchronised once).
 * The handle needs no built index: it provides the device and the stream.  The host plans the join (lmi_range_join_plan.h: pure
 * arithmetic) and range_join_kernel copies: runs are cut into pieces of at most piece_rows results (default 4 096), one block of 256
 * lanes per piece, 4-byte loads and stores (source and target share no alignment), no LDS, no atomic, nothing written outside a
 * piece's target.  Device memory of a call: the result (8 bytes per result), 24 bytes per piece, 16 per part; with host pointers
 * the staged parts (8 bytes per result) while the call runs.
 * Refused before any launch or allocation: a NULL handle; world outside 1..64; nq < 0; nb outside 1..1024; nq * nb >= 2^31; NULL
 * counts, dists or ids with nq > 0; a negative count (names the part, query and t); a (query, t) that two parts both claim (names
 * the query, t and both parts: the parts' ownerships overlap); a part whose total is > 0 with a NULL array; a NULL result pointer;
 * a negative max_total; a grand total above max_total when max_total > 0 (says the total).  *result = NULL after a refusal.
 * nq == 0 succeeds with an empty result (lims = {0}). */
LMI_API int lmi_join_range_parts(lmi_index *h, int world, int nq, int nb, const int32_t *counts /* host, [world][nq][nb] */,
                                 const float *const *dists /* [world] */, const uint32_t *const *ids /* [world] */,
                                 int64_t max_total, lmi_range_result **result, int on_device);
/* The exchange through RCCL inside the library: every rank passes its part (the lmi_range_result of its lmi_scan_range) -> ONE
 * ncclAllGather of the part's nq * nb counts on the handle's stream -> ONE stream synchronisation, so that the host can size the
 * payload and plan the join -> ONE ncclAllGather of [dists | ids], each padded to the largest part's total Tmax (ncclAllGather is the
 * only collective the library resolves and it moves equal blocks: 8 * world * Tmax bytes are received where 8 * total are needed) ->
 * the join, as above.  The joined result is identical on every rank.  nq and nb are the part's; ALL RANKS MUST PASS PARTS OF THE SAME
 * nq AND nb: a mismatch the gathered counts cannot show (they are exchanged in blocks of this rank's nq * nb) is the caller's
 * responsibility.  A part whose total differs from what its gathered counts sum to is refused.
 * Refusals as lmi_join_range_parts, and a NULL part, a NULL communicator, a rank outside 0..world-1; fails cleanly when RCCL is
 * absent.  nq == 0 succeeds with an empty result and no collective. */
LMI_API int lmi_allgather_join_range(lmi_index *h, void *comm, int rank, int world, const lmi_range_result *part, int64_t max_total,
                                     lmi_range_result **result);
/* Test hook: the most results of one copy piece of the joins on this thread; 0 = the default (4 096).  Never changes a bit of a
 * result.  Refused: a negative value, one above 2^30. */
LMI_API int lmi_range_join_set_geometry(int64_t piece_rows);
enum {
    LMI_RANGE_JOIN_PARTS = 0,         /* parts joined: world                                                                  */
    LMI_RANGE_JOIN_RUNS,              /* non-empty (query, t) runs                                                            */
    LMI_RANGE_JOIN_PIECES,            /* copy pieces = blocks of the kernel's grid                                            */
    LMI_RANGE_JOIN_RESULTS,           /* results of the join: lims[nq]                                                        */
    LMI_RANGE_JOIN_LARGEST_PART,      /* the largest part's total (Tmax: what lmi_allgather_join_range pads every part to)    */
    LMI_RANGE_JOIN_COUNT
};
/* What the last join on this thread did (all zero before the first, after a refused or failed call and after one with nq == 0);
 * writes min(n, LMI_RANGE_JOIN_COUNT) words. */
LMI_API int lmi_debug_range_join_plan(int64_t *out, int n);

/* A range result sorted by distance, on the device and in place (no reference counterpart): nearest first, for callers that read the
 * result (lmi_range_result_read, host or device pointers) after the sort.  h provides the device and the stream only and needs no
 * built index, like lmi_join_range_parts; r is any result of that device: a scan's or a join's.  tests/range_sort_ref.py restates the
 * contract in numpy.
 * Contract
 *   order        for every query q with segment [a, b) = [lims[q], lims[q + 1]): dists[a:b] and ids[a:b] are permuted TOGETHER so that
 *                the pairs (key(dist), position the entry had in the segment before the call) ascend.  key orders binary32 values
 *                numerically with -0 == +0; every NaN, of either sign and any payload, sorts behind +inf; equal keys keep their
 *                earlier relative order.  This is numpy's argsort(dists[a:b], kind="stable") applied to both arrays.
 *   bits         the bits of dists and ids are MOVED, never recomputed: -0 stays -0, a NaN keeps its payload.
 *   unchanged    lims, nb and the pair counts.  After a sort the pair counts still say how many results every (query, rank t)
 *                contributed, NOT where they lie: the runs of the ranks are interleaved by distance.
 *   determinism  (key, position) is a total order without equal elements, so the result is the same bit for bit for any tile length,
 *                grouping, grid or algorithm; lmi_range_sort_set_geometry never changes a bit.  Sorting a sorted result is allowed
 *                and changes nothing.
 *   flag         the result remembers that it was sorted: lmi_range_result_sorted writes 1, else 0.  lmi_allgather_join_range refuses
 *                a sorted part by name, because the join needs (rank, row) order: sort the JOINED result.  lmi_join_range_parts takes
 *                raw arrays and cannot know: passing it arrays read from a sorted result is the caller's mistake.
 * How: an entry becomes ONE 64-bit word, (order-preserving image of the key << 32) | position; the words of a segment are unique, so an
 * unstable network yields the stable order.  The host picks a form per segment from lims alone (lmi_range_sort_plan.h):
 *   skipped      0 or 1 entries
 *   wave form    2 .. 256 entries: one wave per segment, four per block, the words in registers
 *   tile form    up to tile_rows = T entries (default 8 192: 64 KiB of words, two blocks per CU): one block per segment, sorted in LDS
 *   long form    above T: tiles of T sorted in LDS into a key buffer, then ceil(log2(tiles)) merge passes between two key buffers, every
 *                pass cut by merge path into output pieces of min(T, 2 048) words, one block each
 * (a T below 512 lowers the wave form's limit to T / 2).  The kernels write a permuted COPY, which is copied back over the segments.
 * Memory: the scratch is allocated and freed by the call, per GROUP of whole consecutive segments: 8 bytes per entry of the group
 * (the copy) + 16 bytes per entry of the group's longest long-form segment (the two key buffers) + 12 bytes per wave- or tile-form
 * segment (the tables).  Groups are cut so that 24 bytes per entry of a group stay within scratch_bytes (default 1 GiB): a bound on
 * the copy and the key buffers.  A segment is never split; one that alone exceeds the budget is a group of its own.  Nothing is kept
 * between calls.  All work is enqueued on h's stream; the call synchronises that stream ONCE PER GROUP and returns when the result is
 * sorted.
 * Failure: a failed allocation names the bytes it wanted, frees what the call allocated and leaves the flag unset.  A group's segments
 * are written back only after all of its kernels were enqueued, so after a failed allocation or launch every segment is either as it
 * was or fully sorted, and a repeated call finishes the job.
 * Refused before any launch or allocation, each by name: a NULL h or r; r on another device than h's; a segment of 2^32 entries or
 * more.  nq == 0, a total of 0 and a result whose segments all hold 0 or 1 entries succeed, launch nothing and set the flag. */
LMI_API int lmi_range_result_sort(lmi_index *h, lmi_range_result *r);
LMI_API int lmi_range_result_sorted(const lmi_range_result *r, int *sorted);
/* Test hook, per thread: tile_rows = T of the sorts on this thread (a power of two in [64, 8 192]) and scratch_bytes = the groups'
 * budget (at most 2^40); 0 = the default.  Never changes a bit of a result.  Refused: a negative value, a tile_rows that is not a
 * power of two in [64, 8 192], scratch_bytes above 2^40; nothing is set then. */
LMI_API int lmi_range_sort_set_geometry(int64_t tile_rows, int64_t scratch_bytes);
enum {
    LMI_RANGE_SORT_PLAN_GROUPS = 0,        /* groups with something to sort = stream synchronisations                          */
    LMI_RANGE_SORT_PLAN_WAVE_SEGMENTS,     /* segments sorted in the wave form                                                 */
    LMI_RANGE_SORT_PLAN_TILE_SEGMENTS,     /* segments sorted in the tile form                                                 */
    LMI_RANGE_SORT_PLAN_LONG_SEGMENTS,     /* segments sorted in the long form                                                 */
    LMI_RANGE_SORT_PLAN_SKIPPED_SEGMENTS,  /* segments of 0 or 1 entries                                                       */
    LMI_RANGE_SORT_PLAN_TILE_ROWS,         /* T                                                                                */
    LMI_RANGE_SORT_PLAN_WAVE_ROWS,         /* the wave form's limit: min(256, T / 2)                                           */
    LMI_RANGE_SORT_PLAN_MERGE_ROWS,        /* words of one merge piece: min(T, 2 048)                                          */
    LMI_RANGE_SORT_PLAN_MAX_PASSES,        /* the most merge passes any segment took (0: no long form)                         */
    LMI_RANGE_SORT_PLAN_SCRATCH_BYTES,     /* copy + key buffers of the largest group                                          */
    LMI_RANGE_SORT_PLAN_RESULTS,           /* entries of the result: lims[nq]                                                  */
    LMI_RANGE_SORT_PLAN_COUNT
};
/* What the last lmi_range_result_sort on this thread did (all zero before the first and after a refused or failed call); writes
 * min(n, LMI_RANGE_SORT_PLAN_COUNT) words. */
LMI_API int lmi_debug_range_sort_plan(int64_t *out, int n);

/* The exact range search through the index (no reference counterpart): every range call above answers "the objects within radius[q]
 * among the buckets that were visited"; this one answers it for EVERYTHING the handle stores, and still skips the buckets that cannot
 * hold an answer.  It discards them by the geometry of the partition: a COVER holds per bucket a centre, a covering radius and a row
 * count, and a PRUNING PASS turns (queries, radii) into the list of buckets whose ball the query's ball may meet.
 * The cover (lmi_cover_create): an opaque object like lmi_filter, made from a built handle; it owns its device arrays and may outlive
 * the handle.  For every bucket b of the index (L buckets; d = the caller's columns -- for LMI_METRIC_L2 the stored -|x|^2/2 column is
 * not part of it):
 *   n_b      the live rows (lmi_bucket_sizes; 0 for a bucket this handle does not own).
 *   c_b [d]  binary32: the mean of the live rows by lmi_kmeans's update rule: e = the smallest integer with max|x| < 2^e over the
 *            finite live values of the whole index (0 for all-zero data; the call takes this maximum itself, in a pass of its own),
 *            q(v) = rint(v * 2^(36-e)), S = the int64 sum of q over the bucket's rows per column, c = (float)((double)S / (double)n_b
 *            * 2^(e-36)).  Integer sums are associative: the centres are the same bits on any grid.  An empty bucket gets zeros.
 *   R_b      binary32: per live row the binary64 chain acc = fma(delta, delta, acc), delta = (double)x[t] - (double)c_b[t], t
 *            ascending from acc = 0, one unsplit chain per row; R2_b = the maximum of the chains; R_b = 0 if R2_b == 0, else
 *            nextafterf((float)sqrt(R2_b), +inf).  A one-row bucket and a bucket of equal rows have R_b = 0 where q loses nothing of
 *            the row (no value below 2^(e-36) steps), since the mean is then the row itself.
 *            A bucket that holds a value that is not finite gets R_b = +inf and is always visited (its centre is unspecified).
 *   cn_b     binary64: sqrt(sum c_b[t]^2), a chain in ascending t.
 * The rows are read where they lie (through the per-bucket tables, as lmi_bucket_read does), in three passes: maximum, sums, radii.
 * lmi_cover_create synchronises the handle's stream and only READS the handle: it is allowed on clone views and while clone views
 * live; it returns when the cover is complete.  A cover holds 4 L d + 16 L bytes of device memory; the call allocates 8 L d + 8 L + 4
 * bytes more while it runs.  A failed allocation names the bytes it wanted and frees everything the call allocated.
 * Refused: a NULL handle or out; an index that is not built; an index that is not stored row-major (lmi_set_prefilter(0),
 * LMI_STORAGE_F16), in lmi_scan_range's words; an index of more than 65535 buckets; a bucket of more than 2^26 rows (the bound of the
 * integer sums, as in lmi_kmeans), by name.
 * lmi_cover_read: HOST pointers, each nullable: centres [L][d], radius [L], counts [L].
 * Validity is lmi_filter's rule: a cover fits the handle it was made from and that handle's clone views, keyed by the layout stamp and
 * the device.  After lmi_buckets_insert / lmi_buckets_delete, on the output of lmi_subset / lmi_regroup / lmi_concat and on any other
 * index it is refused -- the message says "stale" -- and must be made again.
 * The admission rule, one binary64 function with explicit fma (csrc/lmi_cover_plan.h; the kernel and a stand-alone CPU self-test run
 * the same text).  For query q, bucket b, r = (double)radius[q], qn = sqrt(sum q[t]^2) (a chain in ascending t) and
 * u = (d + 8) * 2^-23:
 *   IP   ub = (sum q[t] c_b[t]) + qn R_b, the sum one unsplit chain in ascending t;  m = u (1 + |r| + qn (cn_b + R_b));
 *        b is PRUNED iff ub < 1 - r - m.
 *   L2   dc = sqrt(sum (q[t] - c_b[t])^2), an unsplit chain;  lo = max(0, dc - R_b);  m = u (qn + cn_b + R_b)^2;
 *        b is PRUNED iff lo lo > r + m.
 * b is ADMITTED iff n_b > 0, radius[q] is neither NaN nor -inf, and b is not pruned; a NaN anywhere in the test admits (a NaN query
 * admits every non-empty bucket); a radius of +inf admits every non-empty bucket.  The margin m makes the rule hold against the
 * distance the scan COMPUTES in binary32, not the real one: whenever some live row of b has a computed distance <= radius[q], b is
 * admitted (DESIGN.md 5.14.6 proves it).  Every (query, bucket) verdict is one thread's unsplit chain in a fixed order: the admitted
 * set does not depend on groups, waves or grids.
 * lmi_cover_order: row q of bucket_order [nq][nb] <- the admitted bucket ids in ASCENDING bucket id, then -1 up to nb; counts [nq] <-
 * the number admitted.  Both nullable; with bucket_order == NULL the call only counts (nb is not looked at).  If some query admits
 * more than nb buckets the call is refused -- the message names the first such query, its count and nb -- and NOTHING is written.
 * radius is a HOST float [nq], also with on_device; queries_search, bucket_order and counts are all device pointers or all host
 * pointers.  Refused before any launch: a NULL handle; an index that is not built or not stored row-major; a NULL, stale or foreign
 * cover; nq < 0; with an order, nb < 1 or nq * nb >= 2^31; a NULL queries_search or radius where nq > 0.  nq == 0 succeeds.
 * lmi_search_range_exact: the pruning pass, nb = max(1, max_q counts[q]), then lmi_scan_range's own schedule on that order, unchanged.
 *   result     bit for bit that of lmi_scan_range(h, queries, the order of lmi_cover_order, nb, radius, f, filter_of, max_total):
 *              (bucket, row) order; filters, max_total, lmi_range_result_*, lmi_range_result_sort and the pair counts as there.
 *   complete   every live row of the handle whose scan distance is <= radius[q] (and which query q's filter allows) is in it: as sets
 *              the result is lmi_knn_range over everything the handle stores, with equal distance bits per object.  On a sharded
 *              rank: complete over the buckets the rank owns (lmi_join_range_parts joins the ranks' parts, all made at one nb).
 *   nb_used    (nullable, a HOST int32) <- nb; counts (nullable, [nq]; host or device as on_device says) <- the buckets admitted.
 * Refused, all before any launch or with no result made (*result = NULL): everything lmi_scan_range refuses; a NULL, stale or foreign
 * cover; a query that needs more than 1024 buckets, the scan's limit on nb -- the message names the query and its count.
 * nq == 0 succeeds with an empty result.  The call synchronises the stream once for the counts and then as lmi_scan_range does.
 * Device memory of the pruning pass: 12 nq + 4 min(nq, query_rows) * 2 ceil(L / 64) bytes, and the [nq][nb] order.
 * Not offered: _f16 query forms, lmi_pipeline_submit, a query split over several scans, a norm-interval bound beside the ball, exact
 * k-NN by the same bound, the stored forms that are not row-major. */
typedef struct lmi_cover lmi_cover;
LMI_API int lmi_cover_create(lmi_index *h, lmi_cover **out);
LMI_API int lmi_cover_destroy(lmi_cover *c);
LMI_API int lmi_cover_read(const lmi_cover *c, float *centres /* [L][d], nullable */, float *radius /* [L], nullable */,
                           int64_t *counts /* [L], nullable */);
LMI_API int lmi_cover_order(lmi_index *h, const lmi_cover *c, const float *queries_search, int nq, const float *radius /* host [nq] */,
                            int nb, int32_t *bucket_order /* [nq][nb], nullable */, int32_t *counts /* [nq], nullable */, int on_device);
LMI_API int lmi_search_range_exact(lmi_index *h, const lmi_cover *c, const float *queries_search, int nq,
                                   const float *radius /* host [nq] */, const lmi_filter *f /* nullable */,
                                   const int32_t *filter_of /* host [nq], nullable */, int64_t max_total, lmi_range_result **result,
                                   int32_t *nb_used /* host, nullable */, int32_t *counts /* [nq], nullable */, int on_device);
/* Test hook, per thread: the queries of one group of the pruning pass (0 = the default: 16 384, fewer where a group's bitmap would pass
 * 64 MiB).  Never changes a bit of an order or a result.  Refused: a value outside [0, 2^20]; nothing is set then. */
LMI_API int lmi_cover_set_geometry(int64_t query_rows);
enum {
    LMI_COVER_PLAN_GROUPS = 0,        /* groups the queries were taken in                                                     */
    LMI_COVER_PLAN_QUERY_ROWS,        /* queries per group (the last may be smaller)                                          */
    LMI_COVER_PLAN_BUCKETS,           /* L of the cover                                                                       */
    LMI_COVER_PLAN_ADMITTED,          /* admitted (query, bucket) pairs of the call                                           */
    LMI_COVER_PLAN_MAX_PER_QUERY,     /* the most buckets any query admitted                                                  */
    LMI_COVER_PLAN_NB_USED,           /* nb of the order that was written (0: the call only counted)                          */
    LMI_COVER_PLAN_WORKSPACE_BYTES,   /* device bytes the pruning pass allocated (the order not included)                     */
    LMI_COVER_PLAN_COUNT
};
/* What the last lmi_cover_order / lmi_search_range_exact on this thread did (all zero before the first, after a refused or failed call
 * and after one with nq == 0); writes min(n, LMI_COVER_PLAN_COUNT) words.  lmi_debug_range_plan reports the scan of an exact call. */
LMI_API int lmi_debug_cover_plan(int64_t *out, int n);

/* Timings of the last lmi_mlp_topk / lmi_scan_topk / lmi_search call (synchronises the stream). */
LMI_API int lmi_timings(lmi_index *h, float *ms /* [LMI_T_COUNT] */);
/* Mean of the timing slots over the calls made since lmi_timings_reset (the newest 128 at most), read
 * with ONE stream synchronisation, so a timed loop needs no per-call sync; *n_calls = calls averaged. */
LMI_API int lmi_timings_reset(lmi_index *h);
/* How much is timed, and how.  2 (default): every phase, from stamps of the chip's constant 100 MHz clock that the first / last
 * workgroups of the search's kernels write into a per-handle ring -- no event, no bubble, nothing to wait for.  3: every phase
 * from hipEvents recorded between the kernels (each one is a ~5 us bubble on the stream: 8 of them are 6 % of a 10M x 45 search);
 * 1: hipEvents for LMI_T_TOTAL (and LMI_T_INFERENCE) only; 0: nothing. */
LMI_API int lmi_set_timing(lmi_index *h, int level);
LMI_API int lmi_timings_mean(lmi_index *h, float *ms /* [LMI_T_COUNT] */, int *n_calls /* nullable */);
/* Work done by the last scan: flops = 2 * d * sum over (query, rank) of the bucket size;
 * items = work items executed by the persistent scan kernel. */
LMI_API int lmi_scan_stats(lmi_index *h, double *flops, int64_t *pairs, int64_t *items);
/* Scan mode.  on (default): fp16-MFMA prefilter with a proven error bound + exact binary32
 * re-ranking of the survivors (lmi_prefilter.h); off: every similarity by f32 MFMA.  Both modes
 * return bit-identical results; call before lmi_buckets_begin (the index is stored differently:
 * row-major f32 + fp16 fragments vs f32 fragments).  lmi_prefilter_stats: whether the last scan used the prefilter, how many candidates were
 * re-scored exactly and how many (query, rank) slots fell back to the exact brute-force kernel.  Any other value of
 * `on` is an error. */
LMI_API int lmi_set_prefilter(lmi_index *h, int on);
/* A second handle on the SAME index (no reference counterpart: the reference is single-threaded Python).  The clone
 * borrows the parent's MLP weights, tree and bucket slabs and has per-call workspaces, a stream and timing events of its
 * own, so that two searches can be in flight on one index, one per handle and stream (learnedmetricindex_amd/pipeline.py
 * alternates handles: a batch's kernels start in the tails of the previous batch's).  Destroy the clone before the parent;
 * do not rebuild the parent's index while a clone lives. */
LMI_API int lmi_clone_view(lmi_index *h, lmi_index **out);
/* Developer aid: copies the first `bytes` of a named internal device buffer to host memory: "pf_bound" (pass 1's slot maxima),
 * "pf_stamps" (phase cycles of -DLMI_P2_STAMPS builds), "pf_redo" ([0]: columns whose candidate buffer overflowed in the last scan);
 * "cand_total" (8 bytes): the candidates pass 2 emitted in the last scan, summed over all columns. */
LMI_API int lmi_debug_peek(lmi_index *h, const char *name, void *dst, int64_t bytes);
LMI_API int lmi_prefilter_stats(lmi_index *h, int *active, int64_t *survivors, int64_t *fallbacks);
/* Tuning: rows per scan chunk (multiple of the 256-row block tile).  Not called: lmi_buckets_begin picks
 * 256..2048 by the size of the index (this rank's rows / 4096), and more for buckets beyond 1024 chunks. */
LMI_API int lmi_set_chunk_rows(lmi_index *h, int rows);
/* Device memory (bytes) the per-call workspaces of one lmi_search / lmi_scan_topk of nq queries x n_buckets need on a built
 * index -- the candidate buffers of the prefilter dominate (~10 KiB per (query, bucket) slot).  No reference counterpart (the
 * reference holds no device memory); li/LearnedIndex.py sizes its query chunks from it. */
LMI_API int lmi_workspace_bytes(lmi_index *h, int nq, int n_buckets, int64_t *bytes);

/* Test hooks for the prefilter's error bound (tests/test_gpu_bound.py; no reference counterpart).
 * lmi_debug_emit_all(1): the next scans drop the sampled bound, so pass 2 emits EVERY row of a visited
 * bucket (buckets of <= 1024 rows fit the candidate buffer) -- results are unchanged (overflowing slots take
 * the exact fallback).  lmi_debug_read_candidates: for (query, rank) slot = q*nb + r of the last scan, the
 * in-bucket rows and the fp16-MFMA scores shat pass 2 computed for them (scaled units: shat ~ xscale *
 * qscale * <q, x>), the emitted count (-1: unvisited), 2*eps' of the slot and the two power-of-two scales. */
LMI_API int lmi_debug_emit_all(lmi_index *h, int on);
LMI_API int lmi_debug_read_candidates(lmi_index *h, int64_t slot, int cap, uint32_t *rows, float *shat,
                              int *count, float *eps2, float *qscale, float *xscale);
/* Test hook for the mutation layout (tests/test_gpu_mutate_fuzz.py; no reference counterpart).  Copies the host tables
 * of a built index: rb_start[L + 1] (bucket b's first row-block; [L] = the row-blocks the layout spans), cap_rb[L]
 * (row-blocks reserved per bucket), n_rb_total, alloc_rb (row-blocks every allocation of the slab holds) and counters[4]:
 * buckets that took inserted rows in their slack, buckets relocated behind the last row-block, re-packs that grew the
 * allocations and re-packs whose layout fit the allocations they replaced (forced by holes), summed over the handle's
 * lmi_buckets_insert calls.  Any pointer may be NULL.  Launches nothing and reads no device memory. */
LMI_API int lmi_debug_layout(lmi_index *h, int32_t *rb_start, int32_t *cap_rb, int64_t *n_rb_total, int64_t *alloc_rb,
                             int64_t *counters);
/* Test hooks for the scan's dispatch (tests/test_gpu_seams.py; no reference counterpart): which of its kernel forms a scan takes.
 * The first fourteen words are the call's plan, decided from (handle, nq, n_buckets, k) before the first launch; the rest are the
 * template instances the launch code picks on top of it (-1: that launch is not part of the call). */
enum {
    LMI_PLAN_FAST = 0,            /* fp16 prefilter + exact re-rank; 0: the all-f32 scan                                      */
    LMI_PLAN_LOW_D,               /* the low-dimensional prefilter kernels (K <= 128)                                          */
    LMI_PLAN_PS_WIDE,             /* ... in their wide form                                                                    */
    LMI_PLAN_TILE_CB,             /* col-blocks per query tile                                                                 */
    LMI_PLAN_SAMPLE_MAX,          /* pass 1's largest sampling stride                                                          */
    LMI_PLAN_QBOUND,              /* one bound per query                                                                       */
    LMI_PLAN_PRIMARY_NB,          /* > 0 (= n_buckets): pass 1 samples the primary slots only                                  */
    LMI_PLAN_USE_FRONT,           /* route_kernel + pack_kernel; 0: the separate preparation kernels                           */
    LMI_PLAN_STREAMED,            /* the streamed re-rank; 0: select_rescore_kernel                                            */
    LMI_PLAN_G,                   /* slots of one query per re-rank wave                                                       */
    LMI_PLAN_USE_TAIL,            /* tail_kernel; 0: select_kernel + rescore_kernel x 2                                        */
    LMI_PLAN_TAIL_MERGES,         /* ... which also merges the ranks                                                           */
    LMI_PLAN_KG16,                /* k16-groups of the fp16 fragments                                                          */
    LMI_PLAN_DP,                  /* row pitch (floats) of the re-rank                                                         */
    LMI_PLAN_ROUTE_NB_TEMPLATE,   /* route_kernel<NB>: the specialised rank count, 0 = the generic instance                    */
    LMI_PLAN_PACK_GS,             /* pack_kernel<GS, CP, vec>                                                                  */
    LMI_PLAN_PACK_CP,
    LMI_PLAN_PACK_VEC,
    LMI_PLAN_ROUTE_SORT_GLOBAL,   /* route_group_kernel sorts in a global scratch buffer; 0: in LDS (separate kernels only)    */
    LMI_PLAN_MERGE_KIND,          /* who writes the caller's rows: 0 the fused tail, 1 merge_ranks_kernel, 2 merge_kernel      */
    LMI_PLAN_RESCORE_SMALL_WAVES, /* waves per block of rescore_kernel's small form (select_kernel + rescore_kernel only)      */
    LMI_PLAN_OVERFLOW_SORTED,     /* overflow_rebound_kernel + pass 2's redo launch ran (lmi_debug_last_plan only; else -1)    */
    LMI_PLAN_COUNT
};
/* lmi_debug_last_plan: what the last scan on this handle did, recorded by the scan and its launch sites as they ran (all zero
 * before the first scan; a clone view starts so).  lmi_debug_plan: what a scan of nq queries x n_buckets with this k would do --
 * the same plan function and the same argument checks as lmi_scan_topk; launches nothing and changes nothing.  Both write
 * min(n, LMI_PLAN_COUNT) words. */
LMI_API int lmi_debug_last_plan(lmi_index *h, int32_t *out, int n);
LMI_API int lmi_debug_plan(lmi_index *h, int nq, int n_buckets, int k, int32_t *out, int n);

/* Test hooks for the MLP forward's dispatch (tests/test_gpu_mlp_seams.py; no reference counterpart): which form lmi_mlp_topk /
 * lmi_mlp_proba (and the MLP step of lmi_search / lmi_pipeline_submit) take for a batch.  The words up to LAYERS_QUERIES are the
 * call's plan, decided from (handle, nq, n_buckets, probabilities wanted, logits wanted) before the first launch; the rest are
 * what the launch sites pick on top of it. */
enum {
    LMI_MLP_PLAN_NUM_CUS = 0,     /* compute units of the handle's device: most thresholds below are functions of it           */
    LMI_MLP_PLAN_FM_OK,           /* every model of the handle fits mlp_fused_kernel (hidden widths <= 512)                    */
    LMI_MLP_PLAN_LOGITS_LDS,      /* the last layer's outputs stay in LDS (<= 512 classes); 0: through global memory           */
    LMI_MLP_PLAN_LDS_BYTES,       /* dynamic LDS of a fused block for the current model set                                    */
    LMI_MLP_PLAN_FUSED,           /* a mlp_fused_kernel launch is part of the call                                             */
    LMI_MLP_PLAN_MODE,            /* its instance: 0 TOPK, 1 PROBA, 3 TOPK_STOP, 5 TOPK_ROWS; -1: no fused launch              */
    LMI_MLP_PLAN_FUSED_BLOCKS,    /* its grid (0: none)                                                                        */
    LMI_MLP_PLAN_NQ_HEAD,         /* queries the fused launch takes: nq when the batch is not split, 0 when per-layer only     */
    LMI_MLP_PLAN_LAYERS_QUERIES,  /* queries that go through the mlp_layer_kernel chain: the split's tail, or all, or 0        */
    LMI_MLP_PLAN_CBW0,            /* mlp_layer_kernel<LAST, CBW>: col-blocks per wave of layer i of that chain (1, 2 or 4);    */
    LMI_MLP_PLAN_CBW1,            /* -1: no such launch                                                                        */
    LMI_MLP_PLAN_CBW2,
    LMI_MLP_PLAN_CBW3,
    LMI_MLP_PLAN_CBW4,
    LMI_MLP_PLAN_CBW5,
    LMI_MLP_PLAN_CBW6,
    LMI_MLP_PLAN_CBW7,
    LMI_MLP_PLAN_RANK_KERNEL,     /* the separate ranking launch (behind the per-layer chain, or behind a fused launch whose    */
                                  /* logits went through global memory): 0 rank_classes_kernel, 1 rank_classes_stop_kernel,    */
                                  /* 2 rank_classes_rows_kernel; -1: every query is ranked in the fused kernel's epilogue      */
    LMI_MLP_PLAN_SOFTMAX_KERNEL,  /* softmax_ranked_kernel is part of the call                                                 */
    LMI_MLP_PLAN_VEC_IN,          /* the fused kernel's layer 0 fetches float4 (d % 4 == 0; a partial last chunk is fetched    */
                                  /* element by element all the same); -1: no fused launch                                     */
    LMI_MLP_PLAN_IN_CHUNKS,       /* 96-feature chunks of the fused kernel's layer 0; -1: no fused launch                      */
    LMI_MLP_PLAN_COUNT
};
/* lmi_debug_last_mlp_plan: what the last MLP forward on this handle did, recorded by mlp_enqueue and its launch sites as they ran
 * (all zero before the first one; a refused call records nothing).  lmi_debug_mlp_plan: what a forward of nq queries would do --
 * n_buckets as lmi_mlp_topk takes it (ignored with want_proba), want_proba != 0: lmi_mlp_proba, want_logits != 0: lmi_mlp_topk with
 * its logits output; the same decision function and the same argument checks as the calls; launches nothing and changes nothing.
 * Both write min(n, LMI_MLP_PLAN_COUNT) words. */
LMI_API int lmi_debug_last_mlp_plan(lmi_index *h, int32_t *out, int n);
LMI_API int lmi_debug_mlp_plan(lmi_index *h, int nq, int n_buckets, int want_proba, int want_logits, int32_t *out, int n);

#ifdef __cplusplus
}
#endif
#endif /* LMI_HIP_H */
