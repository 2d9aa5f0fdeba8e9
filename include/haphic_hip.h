/*
 * haphic_hip.h — C ABI of libhaphic_hip.so: MI355X (gfx950) implementation of HapHiC's Hi-C
 * link-matrix construction + Markov clustering hot path (scripts/HapHiC_cluster.py).
 *
 * The reference has no FFI/plugin API; its narrowest seams are module-level Python functions
 * (SURVEY.md §8b, S1–S6).  Every entry point below names the reference interface it replaces
 * (file:line, all in scripts/HapHiC_cluster.py).  The ctypes binding a maintainer would add is
 * haphic_amd/_lib.py; the re-binding of the reference's names is shown in INTEGRATION.md.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; hhx_last_error() gives the
 *     thread-local message (the Python shim raises RuntimeError, as the reference does, e.g. :2507).
 *   - plain pointers and sizes only.  "host" pointers are ordinary memory; "dev" pointers are HIP
 *     device memory on the current device.  Kernels run on the stream set by hhx_set_stream()
 *     (default: the null stream).  ONE stream at a time per process: the library's memory pool recycles blocks in
 *     stream order; hhx_set_stream drains the device when the stream changes, and concurrent callers on different
 *     streams are not supported.
 *   - matrices: the reference's column-stochastic M is scipy CSC (indptr,indices,data) with int32
 *     indices and float32 data.  That triple is byte-for-byte CSR of T = M^T; the library works on
 *     CSR(T).  "row" below == "column" in the reference.  Rows are kept sorted by index.
 *   - hhx_csr is an opaque device-resident matrix owned by the library (release with hhx_csr_free).
 */
#ifndef HAPHIC_HIP_H
#define HAPHIC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hhx_csr hhx_csr;
typedef struct hhx_ingest hhx_ingest;

/* ---------------------------------------------------------------- runtime */
const char *hhx_last_error(void);
int hhx_version(void);
int hhx_device_count(int *count);
int hhx_set_device(int device);
int hhx_set_stream(void *hip_stream);          /* hipStream_t; NULL = null stream (thread-local) */
int hhx_synchronize(void);
int hhx_pool_trim(void);                       /* release cached device memory (a block of hhx_pool_prewarm nobody has used yet survives ONE such call) */
/* the same, but the blocks of at most 64 MiB and, largest first, up to keep_bytes of the blocks of at most 8 GiB stay cached: between two steps of one job the
 * transient blocks of the first (tens of GB at C3) go back to the driver while the second still finds blocks for its own mid-size buffers — a fresh block costs
 * 12-30 ms per GB, and 0.1-0.6 s a call while another thread of the process is releasing memory (measured inside the whole C3 run: DESIGN.md 1.2) */
int hhx_pool_trim_keep(int64_t keep_bytes);
/* take blocks of these sizes from the driver now and leave them in the pool's cache (thread-safe; meant for a helper thread of the caller while a long
 * kernel runs: the next step's pools then cost no fresh device memory).  Stops quietly when the device has no room.  Such a block survives the next
 * hhx_pool_trim (not the one after) unless it has been handed out in between; when the device runs out of memory it is released like every other cached block. */
int hhx_pool_prewarm(int32_t n, const int64_t *bytes);
/* per-kernel device timing with HIP events on the launch stream (bench.py's roofline leg):
 * names: "ingest" (map + partition + aggregate of one push), "aggregate", "ingest_merge", "link_matrix",
 * "spgemm_symbolic", "spgemm_numeric", "expand_window", "expand_window_short", "expand_hash", "expand_compact",
 * "expand_tiny", "inflate_stats", "prune_write", "convergence", "class_layout", "d2m_*" (the stages of the link-matrix
 * build), "bin_contacts" */
/* Which kernel class / arithmetic / layout the calls take (no reference counterpart).  EVERY setting of every knob gives the same
 * results — the verification tests switch classes with them and compare bits; bench.py / tools time the variants.  Known names
 * (anything else is refused): "cls" 0 = stream iteration 0 as (column, value) pairs instead of the class stream; "cls_nc",
 * "cls_balance" (layout of the class stream); "links_integer" 0 = float arithmetic for iteration 0 (results within float32
 * round-off, not the same bits: the other specification of DESIGN.md 2); "links_sym" 0 = every row walks all its products;
 * "dense_tri" 1 / 0 = force / forbid the upper-block-triangle storage of the dense block; "hash_max" = largest product count of a
 * row that tries the LDS hash table first (0: window / compact classes only); "tile_u", "win_batch", "cache_slice_mb" (tile
 * shapes and window count of the window kernel); "block_tiles" 0 = iterations >= 1 of the window class walk the stream in tiles
 * of one (B row, window) segment each instead of 64-entry blocks (default 15; 1, 2, 5, 11, 31: other block-tile shapes /
 * addressings); "row_order" 0 = the window-class rows as listed instead of in min-hash order; "reuse" 4 / 2 = the grouped kernel;
 * "dense_seed_hint" (the sweep's first pool sizes); "correct_agg" 1 = hhx_correct_push merges the atomic adds of the lanes of a wave that hit the
 * same word before they leave the wave (default 0: one atomic per lane; tools/correct_bench.py times both); "plotnorm_small" = the largest
 * block (bins) hhx_plotnorm_balance runs inside one workgroup, clamped to [0, 512] (default 512; 0: every block is steered from the host;
 * the two implementations sum in another order, so the blocks' x agrees within the spread the reference's bnewt shows under a permutation,
 * step counts equal); "plotnorm_chunk_cells" = cells per upload / apply chunk of hhx_plotnorm (default 2^24, at least 1: one row per chunk;
 * same bits); "sort_lds_shape" = the largest new shape whose re-aggregation of hhx_sort_graph_aggregate accumulates in LDS, clamped to [0, 192]
 * (default 192; 0: always global atomics; same bits); "groupstats_lds_slots" = slots of the per-workgroup LDS table of hhx_group_stats /
 * hhx_ingest_group_stats (40 bytes each), rounded down to a power of two in [16, 2048] (default 2048; a contig with more distinct groups than slots takes
 * the table in HBM; same bits; hhx_reassign_round orders a row of that many groups in LDS (20 bytes each) and a wider one in HBM);
 * "reassign_window" = the most contigs of the visiting order one evaluation of hhx_reassign_round judges, clamped to [1, 4096] (default 512; same
 * results, other launch counts); "fasta_slab" = bytes of scaffolds.fa that hhx_fasta_emit produces per kernel launch and hands to the file writer
 * in one piece, rounded down to a multiple of 16 in [256, 2^26] (default 2^26; the same file, other seams); "sort_verdict_lds_n" = the largest n whose
 * rotations hhx_sort_verdict_sums runs with their tree in LDS, clamped to [0, 40959] (4-byte cells: lengths summing to less than 2^32) or [0, 20479]
 * (8-byte cells) (default 4095 / 2047: a tree of 16 KiB, above which a CU holds too few rotations to hide a step's latency; 0: every rotation on its
 * scratch slab in HBM; same bits); "pkl_chunk" = bytes per chunk of the opcode-boundary search of hhx_pickle_open, clamped to [512, 16384] (default 4096;
 * the same arrays, other seams); "heads_bitmap" 0 = hhx_pickle_group_heads gathers the slot of both names of every key instead of testing them
 * against the bitmap of the group's names in LDS first (default 1; tables of more than 2^19 names always gather; same arrays;
 * tools/sort_heads_bench.py times both); "heads_grid" = the most workgroups (four wavefronts each, every wavefront one contiguous range of the table)
 * of the passes of hhx_pickle_group_heads, clamped to [1, 1536] (default 1536; fewer: more steps per wavefront; same arrays); "sort_forest_lds" = the largest shape whose hhx_sort_graph_forest runs as one
 * workgroup on LDS arrays, clamped to [0, 2048] (default 2048; 0: always the multi-launch form in HBM; same arrays); "reassign_check_grid" = the
 * most workgroups of the pass over the keys that hhx_reassign_create_from_pickle runs before it builds a handle, clamped to [1, 2048] (default 2048;
 * fewer: more steps per lane; same answers); "clm_chunk" = the most distances (four per kept read pair) hhx_ingest_write_clm sorts and formats
 * at once, clamped to [4, 2^27] (default 2^27; whole contig pairs per chunk, at least one; read once per file; the same file, other seams);
 * "sink_piece" = bytes per piece the file writer of paired_links.clm, scaffolds.fa and alignments.bed copies to a pinned buffer and hands to
 * its pwrite() threads, clamped to [4096, 2^26] (default 2^26; read once when the file is opened; the same file).  value INT64_MIN: back
 * to the default.  Unset knobs fall back to the
 * environment variable HHX_<NAME>. */
int hhx_tune(const char *name, int64_t value);
int hhx_profile_enable(int on);
int hhx_profile_reset(void);
int hhx_profile_get(const char *kernel, double *total_ms, int64_t *launches);
/* event counters gathered while profiling is on: "expand_window_products" (products streamed by
 * k_expand_window_pass), "expand_window_a_reads" (entries of A staged, summed over the column windows),
 * "ingest_records" (read pairs that survive the map stage); per fused expansion, the rows k_classify puts in each class —
 * "expand_rows_window", "expand_rows_compact", "expand_rows_tiny", "expand_rows_hash" — the hash-class rows the hash kernel hands
 * back ("expand_rows_hash_to_window", "expand_rows_hash_to_compact"), the column windows of the window-class launch
 * ("expand_window_n_win") and the survivor-pool retries ("expand_pool_retries"); per hhx_pairs_parse, the blocks of 128 lines whose
 * text was staged in LDS / read from HBM directly ("text_blocks_staged", "text_blocks_direct": a span beyond the LDS window, or a
 * device buffer that is not 16-byte aligned) and, of the blocks that write alignments.bed bytes, those formatted in LDS / straight
 * into HBM ("bed_blocks_lds", "bed_blocks_direct"); per hhx_ingest_write_clm, the chunks of the file ("clm_chunks") and the blocks of 256
 * distances whose text, beyond the 24 KiB LDS window, went straight into HBM ("clm_blocks_direct"); the pieces every device-fed file left
 * in ("sink_pieces") */
int hhx_profile_counter(const char *name, int64_t *value);

/* ---------------------------------------------------------------- matrices */
/* build from / copy to host arrays (numpy: csc.indptr, csc.indices, csc.data) */
int hhx_csr_from_host(int32_t n_rows, int32_t n_cols, const int32_t *indptr, const int32_t *indices,
                      const float *data, hhx_csr **out);
/* build by copying device arrays (e.g. torch tensors after an all-gather) */
int hhx_csr_from_device(int32_t n_rows, int32_t n_cols, int64_t nnz, const int32_t *dev_indptr,
                        const int32_t *dev_indices, const float *dev_data, hhx_csr **out);
int hhx_csr_shape(const hhx_csr *m, int32_t *n_rows, int32_t *n_cols, int64_t *nnz);
int hhx_csr_to_host(const hhx_csr *m, int32_t *indptr, int32_t *indices, float *data);
int hhx_csr_device_ptrs(const hhx_csr *m, void **dev_indptr, void **dev_indices, void **dev_data);
int hhx_csr_copy(const hhx_csr *m, hhx_csr **out);
/* rows [r0, r1) as a new (r1-r0) x n_cols matrix: the row-block shard of SURVEY §8e */
int hhx_csr_row_block(const hhx_csr *m, int32_t r0, int32_t r1, hhx_csr **out);
/* row blocks stacked in order (same column count; fewer than 2^31 entries in total) */
int hhx_csr_vstack(int32_t n_blocks, const hhx_csr *const *blocks, hhx_csr **out);
/* SURVEY §8e, the per-iteration all-gather(v) of the pruned row blocks (mcl :2026-2062 with T sharded by row block): RCCL has no
 * all-gather-v, so a block travels as ONE int32 message [row lengths | column indices | float32 value bits] padded to the longest
 * message of the world.  hhx_csr_pack_block writes m's message (n_rows + 2 nnz words) into a caller-owned device buffer;
 * hhx_csr_unpack_blocks turns the gathered messages (message b at packed + b * stride_words, rows[b] rows / nnz[b] entries — host
 * arrays, from the header exchange) into the stacked matrix: three device copies per block and one scan for the row pointer. */
int hhx_csr_pack_block(const hhx_csr *m, void *dst_dev, int64_t capacity_words);
int hhx_csr_unpack_blocks(int32_t n_blocks, const int64_t *rows, const int64_t *nnz, const void *packed_dev, int64_t stride_words,
                          int32_t n_cols, hhx_csr **out);
/* free / total device memory in bytes (memory cached by the library's pool counts as used: hhx_pool_trim first) */
int hhx_mem_info(int64_t *free_bytes, int64_t *total_bytes);
/* bytes cached by the library's pool: reusable by the library's next allocations without asking the driver */
int hhx_pool_cached_bytes(int64_t *bytes);
int hhx_csr_free(hhx_csr *m);

/* ---------------------------------------------------------------- S3: normalize / power / prune
 * sklearn.preprocessing.normalize(M, norm='l1', axis=0), call sites :2014 :2038 :2144 — in place. */
int hhx_normalize_l1(hhx_csr *m);
/* `normalize(matrix.power(inflation), norm='l1', axis=0)` :2037-2038 — in place. */
int hhx_inflate(hhx_csr *m, double inflation);
/* prune(matrix, pruning, dense_matrix=False) :1987-2014: keep entries >= pruning, restore the row
 * maximum, L1-normalise. */
int hhx_prune(const hhx_csr *m, double pruning, hhx_csr **out);
/* :2037-2042 fused: prune(normalize(power(C, inflation))); C is consumed (its data is overwritten). */
int hhx_inflate_prune(hhx_csr *c, double inflation, double pruning, hhx_csr **out);
/* same result, c untouched: for a row block of the pre-expanded matrix that run_mcl_clustering's inflation sweep
 * (:2155-2158) revisits for every inflation */
int hhx_inflate_prune_keep(const hhx_csr *c, double inflation, double pruning, hhx_csr **out);

/* ---------------------------------------------------------------- S1: expansion
 * sparse_dot_mkl.dot_product_mkl(A_csc, B_csc) :39-43, used by mkl_matrix_power :2017-2023.
 * On the CSC view out = A_csc * B_csc; in CSR(T) terms the caller passes (a = T_B, b = T_A), i.e.
 * out_T = T_B * T_A.  a may be a row block (n_local x k) of the left operand (multi-GPU shard).
 * Accumulation: each float32 product is formed exactly in double, rounded to the nearest multiple of
 * 2^-fx_shift (ties to even; shift chosen from ||a||_inf * max|b|) and summed exactly (64-bit integer adds),
 * so the result is independent of summation order and of the GPU count; it is rounded to float32 once. */
int hhx_spgemm(const hhx_csr *a, const hhx_csr *b, hhx_csr **out);
/* same with an explicit fixed-point shift (tests); products counted into *n_products if non-NULL */
int hhx_spgemm_ex(const hhx_csr *a, const hhx_csr *b, int fx_shift, hhx_csr **out, int64_t *n_products);

/* One fused MCL iteration on the device, :2030-2042: out = prune(normalize(power(a * b, inflation))),
 * the expanded matrix a*b is consumed row by row in LDS and never written to HBM (at n = 100k the
 * un-pruned pre-expansion of :2147 has 10^10 entries).  a may be a row block.  Operands must be
 * stochastic (entries in [0,1], row sums <= 1): products are rounded on the 2^-fx_shift grid, fx_shift <= 52
 * (default 52), and accumulated with exact float64 adds. */
int hhx_expand_inflate_prune(const hhx_csr *a, const hhx_csr *b, int fx_shift, double inflation, double pruning,
                             hhx_csr **out, int64_t *n_products, int64_t *nnz_expanded);

/* ---------------------------------------------------------------- S2: convergence + whole mcl()
 * :2044-2046  d = abs(M - last) - 1e-5*abs(last); *stat = max(0, d.max()) evaluated in float32. */
int hhx_convergence_stat(const hhx_csr *m, const hhx_csr *last, float *stat);
/* mcl(matrix, expansion, inflation, iters, pruning, dense_matrix=False) :2026-2062 on the
 * pre-expanded matrix (run_mcl_clustering :2144-2147).  Not converging is not an error (:2058-2062):
 * *converged = 0 and the last matrix is returned.  stats (may be NULL) receives 4 int64 per executed
 * iteration: nnz entering, nnz after expansion, nnz after pruning, number of products. */
int hhx_mcl(const hhx_csr *pre_expanded, int expansion, double inflation, int max_iter, double pruning,
            hhx_csr **out, int *n_iter, int *converged, int64_t *stats);
/* run_mcl_clustering :2144-2158 for one inflation, starting from the L1-normalised link matrix: the
 * pre-expansion (:2146-2147) is fused into iteration 0 instead of being materialised. */
/* mcl() :2026-2062 picked up after its first `done` (>= 1) iterations, `m` being the matrix they left; n_iter and
 * stats[] keep counting from `done`.  run_mcl_clustering at orders where M^e has more than 2^31 entries keeps M^e in
 * HBM as row blocks (hhx_spgemm on hhx_csr_row_block), forms iteration 0 of every inflation with
 * hhx_inflate_prune_keep per block + hhx_csr_vstack, and resumes here: the expansion of the link matrix (a second
 * per inflation at n = 100k) is paid once for the whole sweep, as in the reference (:2146-2147). */
int hhx_mcl_resume(const hhx_csr *m, int done, int expansion, double inflation, int max_iter, double pruning,
                   hhx_csr **out, int *n_iter, int *converged, int64_t *stats);
int hhx_mcl_normalized(const hhx_csr *normalized, int expansion, double inflation, int max_iter, double pruning,
                       hhx_csr **out, int *n_iter, int *converged, int64_t *stats);
/* The inflation sweep of run_mcl_clustering :2155-2158 (every inflation restarts from the matrix pre-expanded at :2146-2147) with ONE
 * expansion.  hhx_expand_links_dense: rows [r0, r1) of M^2 — M the L1-normalised (:2144) raw link matrix of dict_to_matrix — as a
 * dense float32 row block in HBM (4 B x (r1 - r0) x n; all rows of a symmetric integer matrix whose square does not fit: the upper block
 * triangle alone, 0.55 x 4 B x n^2; hhx_dense_shape reports the bytes).  hhx_dense_inflate_prune: iteration 0 of
 * mcl() (:2037-2042: power, normalise, prune, restore the maximum, normalise) of those rows at one inflation, bit for bit what
 * hhx_mcl_links computes in its first iteration; stack the blocks (hhx_csr_vstack) and continue with hhx_mcl_resume(done = 1). */
typedef struct hhx_dense hhx_dense;
/* upper_only = 1 (integer arithmetic only): fill just the blocks (I, J >= I) of the rows — 60 % of their products — and leave the
 * columns left of a row's own block to the caller, who owns the mirror image: the ranks of the multi-GPU driver exchange them
 * (hhx_dense_device gives the block and its column-window plan).  hhx_links_integer_ok says whether the arithmetic applies. */
int hhx_expand_links_dense(const hhx_csr *links, int32_t r0, int32_t r1, int fx_shift, int upper_only, hhx_dense **out,
                           int64_t *n_products, int64_t *nnz_expanded);
int hhx_links_integer_ok(const hhx_csr *links, int *ok, int *shift);
/* what iteration 0 of hhx_mcl_links will do with this matrix on this device: *integer (the arithmetic above applies); *layout = 1 the
 * symmetric half into the square float32 block of all rows (+ transposition), 2 into its upper block triangle alone (the square
 * would take too large a share of the device), 0 every row walks all its products into the fused epilogue */
int hhx_links_plan(const hhx_csr *links, int *integer, int *layout);
int hhx_dense_device(const hhx_dense *d, void **x_dev, int64_t *ld, int32_t *cap_win, int32_t *n_win);   /* ld: row pitch in floats (>= n_cols) */
/* rectangles of such a block on their way between ranks (device pointers, sizes and pitches in floats): hhx_copy_rect_f32 packs /
 * places a rows x cols rectangle, hhx_transpose_f32 writes its transpose (dst is cols x rows) — the mirror image of the symmetric
 * pre-expansion, which a rank receives as another rank's rows */
int hhx_copy_rect_f32(const void *src, int64_t src_ld, void *dst, int64_t dst_ld, int64_t rows, int64_t cols);
int hhx_transpose_f32(const void *src, int64_t src_ld, void *dst, int64_t dst_ld, int64_t rows, int64_t cols);
int hhx_dense_inflate_prune(const hhx_dense *d, double inflation, double pruning, hhx_csr **out);
/* the same for k <= 8 inflations in ONE pass over the block (x = y / d_i and log2(x) are formed once per entry, the 4 B x n^2 block
 * is read once): outs[i] is bit for bit what hhx_dense_inflate_prune(d, inflations[i], ...) returns */
int hhx_dense_inflate_prune_multi(const hhx_dense *d, int k, const double *inflations, double pruning, hhx_csr **outs);
int hhx_dense_shape(const hhx_dense *d, int32_t *n_rows, int32_t *n_cols, int64_t *bytes);
int hhx_dense_free(hhx_dense *d);

/* run_mcl_clustering :2144-2158 for one inflation straight from the RAW link matrix that dict_to_matrix
 * returns (:362-368): the L1 normalisation (:2144), the pre-expansion (:2146-2147, fused into iteration 0) and
 * mcl().  When the matrix holds integer link counts <= 65535 (always, unless --normalize_by_nlinks / GFA weights
 * were applied) iteration 0 streams its right operand as the CLASS STREAM: the count-1 entries of every (row, column
 * window) segment — 75 % of a Hi-C link matrix — go as 16-bit columns alone, 2 B per product instead of 6.
 * When it is also SYMMETRIC with row sums below 2^18 (every matrix of dict_to_matrix at the sizes of BASELINE.json) the
 * pre-expansion runs in INTEGER arithmetic, (M^2)_ij = S_ij / d_i with S = L D^-1 L evaluated exactly (DESIGN.md
 * 4.1; within 3e-7 of the float32-normalised product, far inside the float32 accumulation noise of the
 * reference's own SpGEMM): S is symmetric bit for bit, so only its upper block triangle is computed and the rest is
 * transposed — 60 % of the products at five column windows.  Other matrices take the float arithmetic of
 * hhx_normalize_l1 + hhx_mcl_normalized (bit-identical to it). */
int hhx_mcl_links(const hhx_csr *links, int expansion, double inflation, int max_iter, double pruning,
                  hhx_csr **out, int *n_iter, int *converged, int64_t *stats);
/* products_host[i] = sum over the entries (i, k) of a of nnz(row k of b): the cost of row i of a * b.  The multi-GPU driver
 * cuts the row blocks of the expansion at equal product counts with it (SURVEY §8e "row-block ... by balanced nnz"). */
int hhx_row_products(const hhx_csr *a, const hhx_csr *b, int64_t *products_host);
/* Iteration 0 of hhx_mcl_links for ONE ROW BLOCK (multi-GPU shard): rows [r0, r1) of the result, links = the WHOLE raw
 * link matrix (all-gathered).  Same arithmetic, hence the same bits, as the one-GPU call (a row block cannot use the symmetry:
 * it walks all its products). */
int hhx_expand_links(const hhx_csr *links, int32_t r0, int32_t r1, int fx_shift, double inflation, double pruning,
                     hhx_csr **out, int64_t *n_products, int64_t *nnz_expanded);

/* ---------------------------------------------------------------- --dense_matrix (:2723): the reference's numpy mode of mcl()
 * hhx_dmat: an n x n float32 matrix M in HBM, the column-stochastic operand of the dense recurrence (hhx_dense above is something else:
 * rows of M^2 of the SPARSE sweep).  Stored as T = M^T row-major in an ld x ld block (ld = n rounded up to 128) whose entries outside
 * n x n are always zero (csrc/hhx_densemcl.hip); every array that crosses this interface is M as the reference has it.  Products are
 * float32 in, float32 accumulate, one accumulator per element with k ascending (v_mfma_f32_32x32x2_f32: an fmaf chain, the same bits on
 * every launch); sums of a column are float32 in one fixed order.  Memory comes from the pool: mcl() with expansion 2 holds the input,
 * the matrix and its product (one block more from expansion 3 on); a block that does not fit is an error that names its size. */
typedef struct hhx_dmat hhx_dmat;
/* m: n x n float32, row-major, M itself (numpy: the C-contiguous array `matrix`) */
int hhx_dmat_from_host(int32_t n, const float *m, hhx_dmat **out);
/* t: CSR(T) == the reference's CSC(M), as dict_to_matrix :362-368 leaves it on the device; `.toarray()` without the host */
int hhx_dmat_from_csr(const hhx_csr *t, hhx_dmat **out);
int hhx_dmat_to_host(const hhx_dmat *m, float *out);                    /* out: n x n float32, row-major, M */
/* the non-zero entries as CSR(T), columns ascending: hhx_interpret (:2065-2095, the dense branch :2080 picks the same entries) and
 * to_scipy_csc serve the result unchanged */
int hhx_dmat_to_csr(const hhx_dmat *m, hhx_csr **out);
int hhx_dmat_copy(const hhx_dmat *m, hhx_dmat **out);                   /* matrix.copy() :2003 :2057 */
int hhx_dmat_shape(const hhx_dmat *m, int32_t *n, int64_t *ld, int64_t *bytes);     /* any of the three may be NULL */
int hhx_dmat_free(hhx_dmat *m);
/* out = a @ b (numpy matmul of the two M; on the stored transposes T_b * T_a): the bare product of matrix_power :2035 :2149 */
int hhx_dmat_gemm(const hhx_dmat *a, const hhx_dmat *b, hhx_dmat **out);
/* normalize(matrix, norm='l1', axis=0) :2144 in place: every column divided by its float32 sum of absolute values; a zero column stays */
int hhx_dmat_normalize_l1(hhx_dmat *m);
/* prune(matrix, pruning, dense_matrix=True) :1999-2014: entries < pruning zeroed, the FIRST maximum of every column of the un-pruned
 * matrix (argmax(axis=0) :2012) put back whatever its value, columns L1-normalised */
int hhx_dmat_prune(const hhx_dmat *m, double pruning, hhx_dmat **out);
/* numpy.linalg.matrix_power(matrix, expansion) :2035 :2149 in numpy's association order: 1 the matrix, 2 M@M, 3 (M@M)@M, from 4 on the
 * binary decomposition (z = z@z per bit, result = result@z for the set bits, lowest first) */
int hhx_dmat_power(const hhx_dmat *m, int expansion, hhx_dmat **out);
/* mcl(matrix, expansion, inflation, iters, pruning, dense_matrix=True) :2026-2062 on the pre-expanded matrix of :2144-2149: per round
 * matrix_power (not in round 0), power + normalize :2040, prune :2042, and from the third round on allclose(matrix, last_matrix) :2051
 * (|a - b| <= 1e-8 + 1e-5 |b| on every entry, float32).  *n_iter: rounds done when it stopped (n + 1 of :2052, max_iter when it did not
 * converge).  done = the rounds already applied to the input (0: a fresh pre-expanded matrix); done = k with max_iter = k + 1 applies
 * exactly round k (cf. hhx_mcl_resume).  A resumed call has no last_matrix: it never reports convergence in its first round. */
int hhx_dmat_mcl(const hhx_dmat *pre_expanded, int done, int expansion, double inflation, int max_iter, double pruning, hhx_dmat **result,
                 int *n_iter, int *converged);

/* ---------------------------------------------------------------- a12: interpret_result :2065-2095
 * Array half: attractors (ascending) = rows with a non-zero diagonal; members of attractor a =
 * rows of CSR(T) holding column a (ascending).  att[n], att_ptr[n+1], members[nnz] are host
 * buffers.  The set-of-tuples and the partition check (:2084-2095) stay in Python. */
int hhx_interpret(const hhx_csr *m, int32_t *att, int32_t *att_ptr, int32_t *members, int32_t *n_att);

/* ---------------------------------------------------------------- S4: dict_to_matrix :310-373
 * Input: the flank table in dict-insertion order (frag id pairs + value, device or host per
 * `on_device`), frag_set membership flags, n_rest = number of link-less members of frag_set (their
 * indices follow the linked ones; their order is CPython's set order and stays in Python).
 * Output: CSR(T) with self-loops (value 1) when add_self_loops, and frag_index[n_frag] (host; -1 =
 * not linked).  Index assignment = first appearance scanning the items in order, i before j. */
int hhx_dict_to_matrix(int64_t n_keys, const int32_t *frag_i, const int32_t *frag_j, const double *value,
                       int on_device, int32_t n_frag, const uint8_t *in_set_host, int32_t n_rest,
                       int add_self_loops, int32_t *frag_index_host, int32_t *n_linked, hhx_csr **out);

/* ---------------------------------------------------------------- a6: link weights on the flank table
 * The in-place dict rewrites between the ingest and dict_to_matrix, on the (frag_i, frag_j, value) arrays in dict order
 * (host arrays, or the device arrays of hhx_ingest_flank_device with on_device = 1: the weights then never leave HBM
 * on their way into hhx_dict_to_matrix).  value is float64 as in the reference (cast to float32 at :368).
 *   mode 0  normalize_by_nlinks :718-724: value /= (links[i] * links[j]) ** 0.5; per_frag_host = frag_link_dict totals [n_frag]
 *   mode 1  normalize_by_length :727-738 (dead code in the reference): value /= (fl_i / 1e6) * (fl_j / 1e6),
 *           fl = min(length, param), param = 2 * flank in bp; per_frag_host = fragment lengths [n_frag]
 *   mode 2  reduce_inter_hap_HiC_links :695-707: value -= value * param (param = phasing_weight) where tag_host[i] != tag_host[j]
 *           (the haplotype tag read_depth_dict[frag][0] mapped to integers); *n_zero = number of entries that reached 0 —
 *           the reference deletes those from the dict, the caller compacts them out. */
int hhx_link_weights(int64_t n_keys, const int32_t *frag_i, const int32_t *frag_j, double *value, int on_device, int mode,
                     int32_t n_frag, const int64_t *per_frag_host, const int32_t *tag_host, double param, int64_t *n_zero);

/* ---------------------------------------------------------------- f3: reassign's per-group link sums
 * HapHiC_reassign.py parse_link_dict :217-263 (normalize_by_nlinks = False): for every contig pair (i, j) of full_link_dict,
 * in dict order, sums[i][group[j]] += links and sums[j][group[i]] += links (group -1 = 'ungrouped': skipped).  links are
 * integer counts (64-bit integer adds: exact, order-free).  sums_host / first_host: [n_ctg][n_groups]; first = dict
 * position (2 * key index + side) of the first contribution to the cell, -1 (all bits set) if none — the order in which
 * the reference's inner dicts received their keys. */
int hhx_group_link_sums(int64_t n_keys, const int32_t *frag_i, const int32_t *frag_j, const int64_t *links, int32_t n_ctg,
                        const int32_t *group_host, int32_t n_groups, int64_t *sums_host, int64_t *first_host);

/* ---------------------------------------------------------------- a5: restriction-site counts
 * count_RE_sites :75-84 for many segments of one sequence buffer (host bytes, letter case as the caller's
 * parse_fasta :87-113 leaves it): counts[s] = sum over sites of seq[off[s] : off[s]+len[s]].count(site),
 * Python str.count semantics (non-overlapping, leftmost first).  `sites` holds the n_sites patterns after
 * parse_RE_sites' N expansion (:56-72), concatenated; site_len their lengths (<= 32).  Segments may overlap:
 * stat_fragments :188-296 asks for whole contigs, bins and the flank prefix / suffix of either. */
int hhx_count_re_sites(const uint8_t *seq_host, int64_t seq_len, int64_t n_seg, const int64_t *seg_off,
                       const int64_t *seg_len, int32_t n_sites, const uint8_t *sites, const int32_t *site_len,
                       int64_t *counts_host);

/* ---------------------------------------------------------------- f1: filter_fragments rank sums :866-892
 * m: the link matrix WITHOUT self loops (dict_to_matrix(flank_link_dict, filtered_frags) :868).  The reference
 * ranks the fragments of every dense row by links descending (stable: ties and link-less fragments by index),
 * takes the topN of fragment f and sums min(rank_a(b), rank_b(a)) over the unordered pairs of that top list.
 * rank_sum_host[n]: the statistic for every row, computed on the sparse rows (no dense matrix, no sort). */
int hhx_rank_sums(const hhx_csr *m, int topN, int64_t *rank_sum_host);

/* ---------------------------------------------------------------- S5: ingest
 * parse_alignments_for_ctgs :1596-1655 (bins = 0) and parse_alignments :1658-1752 (bins = 1) on
 * integer ids.  The Python shim maps names to ids once (haphic_amd/cluster.py: FragTable):
 *   contig id c in [0,n_ctg); ctg_rank[c] = rank of the contig NAME under Python string order
 *   (key orientation :1629); a split contig owns nbins consecutive fragment ids from ctg_frag0[c];
 *   frag_rank[f] = rank of the fragment NAME (:1720); frag_nx[f] = membership in Nx_frag_set.
 * A contig id < 0 (or >= n_ctg) = name absent from fa_dict (:1625).
 * Positions are 0-based int32 as yielded by the generators (:1556 :1593).
 */
typedef struct {
    int32_t n_ctg, n_frag;
    const int32_t *ctg_rank;     /* [n_ctg]  host */
    const int64_t *ctg_len;      /* [n_ctg]  host */
    const int32_t *ctg_frag0;    /* [n_ctg]  host */
    const uint8_t *ctg_split;    /* [n_ctg]  host */
    const int32_t *frag_rank;    /* [n_frag] host */
    const int64_t *frag_len;     /* [n_frag] host */
    const uint8_t *frag_nx;      /* [n_frag] host */
    int64_t bin_size;            /* only when bins */
    int64_t flank;               /* bp (args.flank * 1000) */
    int32_t bins;                /* 0: parse_alignments_for_ctgs, 1: parse_alignments */
    int32_t skip_intra;          /* 1: drop ref == mref like pairs_generator_inter_ctgs :1582 */
    int64_t expected_keys;       /* unused (kept for ABI stability): the tables are sized on the device */
} hhx_ingest_config;

int hhx_ingest_create(const hhx_ingest_config *cfg, hhx_ingest **out);
/* global stream ordinal of this handle's first pair: rank r of a multi-GPU job passes the number of pairs
 * held by ranks < r, so that first-seen ordinals are comparable across ranks.  Before the first push. */
int hhx_ingest_set_ordinal_base(hhx_ingest *h, int64_t base);
/* one batch of read pairs in stream order (at most 2^32 - 2 per call); id/pos arrays are device
 * (on_device=1) or host memory.  Each push is aggregated on the device into one run of distinct keys. */
int hhx_ingest_push(hhx_ingest *h, int64_t n_pairs, const int32_t *id1, const int32_t *pos1,
                    const int32_t *id2, const int32_t *pos2, int on_device);
/* the same with 64-bit positions: contigs of 2^31 bp and more, where the reference switches its coordinate arrays to int64
 * (determine_int_type :116-147).  With hhx_ingest_keep_pairs on, positions must stay below 2^32 - 1 (32-bit side records). */
int hhx_ingest_push64(hhx_ingest *h, int64_t n_pairs, const int32_t *id1, const int64_t *pos1, const int32_t *id2,
                      const int64_t *pos2, int on_device);
/* close the stream: merges the runs into one table per dict; the numbers of keys are returned */
int hhx_ingest_finalize(hhx_ingest *h, int64_t *n_full_keys, int64_t *n_flank_keys);
/* host copies, in dict insertion order: full_link_dict keys/counts, the HT_link_dict counts of each
 * contig pair ([HH, HT, TH, TT] :404-416), flank_link_dict keys/counts, per-fragment flank link totals
 * (frag_link_dict).  Any pointer may be NULL.  The insertion order is materialised on the first call. */
int hhx_ingest_fetch(hhx_ingest *h, int32_t *full_i, int32_t *full_j, int64_t *full_cnt, int64_t *ht_cnt,
                     int32_t *flank_i, int32_t *flank_j, int64_t *flank_cnt, int64_t *frag_links);
/* device-resident flank table (insertion order) for hhx_dict_to_matrix(on_device=1) */
int hhx_ingest_flank_device(hhx_ingest *h, void **dev_frag_i, void **dev_frag_j, void **dev_value_f64);
int hhx_ingest_flank_count_device(hhx_ingest *h, void **dev_count_i64);   /* same rows, int64 counts */
/* dict_to_matrix :310-373 fused onto the handle's flank table (hhx_dict_to_matrix semantics; the dict
 * insertion order is taken from the first-seen ordinals and never materialised).  n_rest < 0: every
 * link-less member of in_set gets a trailing index (their relative order is CPython's set order and is
 * decided by the Python caller). */
int hhx_ingest_link_matrix(hhx_ingest *h, const uint8_t *in_set_host, int32_t n_rest, int add_self_loops,
                           int32_t *frag_index_host, int32_t *n_linked, hhx_csr **out);
/* Side products that need the read pairs themselves.  hhx_ingest_keep_pairs(h, 1) before the first
 * push keeps, for every pair counted in full_link_dict, its oriented 1-based contig coordinates.  After finalize,
 * hhx_ingest_fetch_pairs returns, per contig pair in dict insertion order (the order of hhx_ingest_fetch):
 *   clm[4 * n]: update_clm_dict :395-401, four distances per read pair, read pairs in stream order;
 *               clm_ptr[k] .. clm_ptr[k+1] are the READ PAIRS of key k (multiply by 4 for the array offset);
 *   crd[2 * m]: record_coord_pairs :454-459, the first max_read_pairs (coord_i, coord_j) of every key.
 * Host buffers: clm_ptr, crd_ptr [n_full + 1]; clm [4 * sum(full_cnt)]; crd [2 * sum(min(full_cnt, max))]. */
int hhx_ingest_keep_pairs(hhx_ingest *h, int on);
int hhx_ingest_fetch_pairs(hhx_ingest *h, int64_t max_read_pairs, int64_t *clm_ptr, int64_t *clm, int64_t *crd_ptr,
                           int64_t *crd);
/* ------------------------------------------------------------------ multi-GPU build of the link matrix
 * dict_to_matrix :310-373 over a pair stream that is split into per-rank chunks.  The matrix index of a fragment is
 * the rank of its first position (2 * first ordinal + side) over the WHOLE stream — a minimum, so the ranks
 * all-reduce(min) hhx_shard_first's array, rank it with hhx_rank_first (same result everywhere), and exchange matrix
 * entries by row owner (all-to-all(v) of hhx_shard_emit's arrays, counts[] entries for each owner) instead of whole
 * tables; hhx_rows_from_entries adds up the counts of equal (row, column) received from different chunks and writes
 * the owner's CSR row block [r0, r1) x shape (self loops :362-364, link-less rows :357-359 at the tail).
 * Entries: w0 = row << 29 | column, w1 = count (uint64 each).  first: int64[n_frag], INT64_MAX = no entry here. */
typedef struct hhx_shard hhx_shard;
int hhx_shard_create(hhx_ingest *h, const uint8_t *in_set, hhx_shard **out);           /* after hhx_ingest_finalize */
int hhx_shard_first(hhx_shard *s, void **first_dev);
int hhx_rank_first(int32_t n_frag, const void *first_dev, void *frag_index_dev, int32_t *n_linked);
int hhx_shard_emit(hhx_shard *s, const void *frag_index_dev, int32_t n_bounds, const int32_t *row_bounds,
                   void **w0_dev, void **w1_dev, int64_t *counts);
int hhx_rows_from_entries(int64_t n, const void *w0_dev, const void *w1_dev, int32_t r0, int32_t r1, int32_t shape,
                          int add_self_loops, hhx_csr **out);
/* the same row block from the received entries AS THE ALL-TO-ALL(V) DELIVERS THEM: n_runs runs (one per source rank; run k =
 * entries [run_off[k], run_off[k + 1]), run_off a host array), each in row order as hhx_shard_emit wrote it — no partition pass */
int hhx_rows_from_runs(int32_t n_runs, const int64_t *run_off, const void *w0_dev, const void *w1_dev, int32_t r0, int32_t r1, int32_t shape,
                       int add_self_loops, hhx_csr **out);
int hhx_shard_destroy(hhx_shard *s);

/* ------------------------------------------------------------------ a1: .pairs text -> id / position arrays
 * pairs_generator :1539-1559 and pairs_generator_inter_ctgs :1562-1583: skip blank and '#' lines, split on
 * whitespace, (ref, pos, mref, mpos) = (cols[1], int(cols[2]) - 1, cols[3], int(cols[4]) - 1), and the two
 * alignments.bed records per line (:1557).  Names are resolved against the FASTA names given at creation
 * (n_names strings, concatenated, name_off[n_names + 1]); a name that is not among them, and every skipped
 * line, yields id -1 — which hhx_ingest_push drops (:1610 / :1702) — so line k of the chunk is element k of
 * the arrays.  A chunk must hold whole lines.  A line with fewer than 5 columns or a malformed integer fails
 * the call with "IndexError: ..." / "ValueError: ..." in hhx_last_error(), as the reference raises, :1556 evaluated
 * left to right (no second column: IndexError; malformed third: ValueError; no fourth or fifth: IndexError;
 * malformed fifth: ValueError), for the first such line of the chunk.  This path's own refusals come after those: a
 * position outside int32 (wide mode: a literal beyond 2^40 in magnitude) is a "ValueError: ...".  The
 * arrays (device pointers, int32) stay valid until the next parse on the same parser. */
typedef struct hhx_pairs_parser hhx_pairs_parser;
int hhx_pairs_parser_create(int32_t n_names, const uint8_t *names, const int64_t *name_off, hhx_pairs_parser **out);
int hhx_pairs_parse(hhx_pairs_parser *p, const uint8_t *text, int64_t n_bytes, int on_device, int want_bed,
                    int64_t *n_lines, int64_t *bed_bytes);
int hhx_pairs_parser_arrays(hhx_pairs_parser *p, void **id1, void **pos1, void **id2, void **pos2, void **bed);
int hhx_pairs_parser_fetch(hhx_pairs_parser *p, int32_t *id1, int32_t *pos1, int32_t *id2, int32_t *pos2, uint8_t *bed);
/* wide mode: positions as int64 from the next parse on (contigs beyond 2^31 bp, :116-147): hhx_pairs_parser_arrays then hands out
 * int64 position arrays (for hhx_ingest_push64), hhx_pairs_parser_fetch64 copies them; ids, BED bytes and errors as before */
int hhx_pairs_parser_set_wide(hhx_pairs_parser *p, int on);
int hhx_pairs_parser_fetch64(hhx_pairs_parser *p, int32_t *id1, int64_t *pos1, int32_t *id2, int64_t *pos2, uint8_t *bed);
/* the alignments.bed bytes of the last parse in pinned host memory owned by the parser: two buffers used in turn, so the
 * pointer stays valid until the SECOND following call (the caller writes buffer k to the file while chunk k + 1 is parsed) */
int hhx_pairs_parser_bed_host(hhx_pairs_parser *p, void **host, int64_t *n_bytes);
int hhx_pairs_parser_destroy(hhx_pairs_parser *p);
/* the .pairs file as chunks of whole lines in PINNED host memory (what pairs_generator* :1543 / :1566 iterate line by line): read with pread() by
 * n_threads (<= 0: 4) threads into one of two buffers while the caller tokenises the other; a chunk holds at most ~2 x chunk_bytes and ends after its
 * last line break.  hhx_text_reader_next: *host is valid until the next call; *n_bytes == 0 at the end of the file.  hhx_pairs_parse(on_device = 0)
 * takes such a chunk to the device at PCIe rate. */
typedef struct hhx_text_reader hhx_text_reader;
int hhx_text_reader_open(const char *path, int64_t chunk_bytes, int n_threads, hhx_text_reader **out);
/* the same over a bgzipped file (`bgzipped_pairs`: gzip.open in the reference :1541 / :1564): BGZF blocks inflated by n_threads threads straight into the
 * pinned buffer.  A file that is not BGZF (a plain gzip stream has no block boundaries to inflate in parallel) is refused: the caller keeps its gzip reader. */
int hhx_text_reader_open_bgzf(const char *path, int64_t chunk_bytes, int n_threads, hhx_text_reader **out);
/* one rank's share of the file (haphic_amd/ranks.py): the lines whose first byte lies in [begin, end) — a boundary inside a line moves forward past
 * the next '\n', so the ranges [b_r, b_{r+1}) of consecutive boundaries hand out every line once, in order; a range may be empty.  bgzf != 0: begin /
 * end are COMPRESSED offsets, the range owns the BGZF blocks that start in it and the same line rule applies to their inflated text. */
int hhx_text_reader_open_range(const char *path, int64_t begin, int64_t end, int64_t chunk_bytes, int n_threads, int bgzf, hhx_text_reader **out);
/* the bytes of the file as they are, chunk_bytes per chunk (the last one shorter), cut anywhere and nothing carried: for a consumer that keeps its own
 * state across cuts (hhx_clm_split_file), so that a line of any length passes. */
int hhx_text_reader_open_raw(const char *path, int64_t chunk_bytes, int n_threads, hhx_text_reader **out);
int hhx_text_reader_next(hhx_text_reader *r, const uint8_t **host, int64_t *n_bytes);
int hhx_text_reader_close(hhx_text_reader *r);
/* measurement only — the writer counterpart of hhx_pairs_parse for synthetic read pairs ("pairs written as .pairs text"): line k =
 * "r{first_read + k}\t{names[id1[k]]}\t{pos1[k] + 1}\t{names[id2[k]]}\t{pos2[k] + 1}\t+\t-\n" from device arrays (ids must be valid: 0 <= id < n_names).
 * *n_bytes = the size of the text; dev_text == NULL: only that.  Not on the product path. */
int hhx_pairs_format(hhx_pairs_parser *p, int64_t n, const int32_t *dev_id1, const int32_t *dev_pos1, const int32_t *dev_id2, const int32_t *dev_pos2,
                     int64_t first_read, uint8_t *dev_text, int64_t capacity, int64_t *n_bytes);

/* ------------------------------------------------------------------ f4: BAM front end
 * bam_generator :1586-1593 = pysam.AlignmentFile(bam, threads=..., format_options=[b'filter=...']) yielding
 * (reference_name, next_reference_name, reference_start, next_reference_start) per record that passes the htslib filter
 * ('flag.read1' :2837 :2855, 'flag.read1 && refid != mrefid' :2862).  hhx_bam_open reads the BGZF container and the BAM
 * header (SAM text for check_sorting_order :1347-1359; reference names, concatenated, name_off[n_ref + 1]).
 * hhx_bam_next inflates the next batch of BGZF blocks (host threads), walks the record lengths and decodes the batch on the
 * device: record k of the batch = element k of four int32 device arrays (valid until the next call), ids mapped through
 * ref_to_ctg_host[n_ref] (BAM reference id -> contig id of the FASTA, -1 = not in fa_dict), records that fail the filter
 * (flag & need_flags != need_flags; or refID == next_refID when drop_same_ref) carry id -2 in both columns, unmapped ends
 * and references outside the map id -1 — hhx_ingest_push drops every negative id, as `ref not in fa_dict` does
 * (:1610 / :1702).  *n_records == 0: end of file. */
typedef struct hhx_bam hhx_bam;
int hhx_bam_open(const char *path, int threads, hhx_bam **out);
int hhx_bam_header(hhx_bam *b, int32_t *n_ref, const char **text, int64_t *text_len, const char **names, const int64_t **name_off);
int hhx_bam_next(hhx_bam *b, int need_flags, int drop_same_ref, int32_t n_ref, const int32_t *ref_to_ctg_host, int64_t max_inflated_bytes,
                 int64_t *n_records, void **id1_dev, void **pos1_dev, void **id2_dev, void **pos2_dev);
int hhx_bam_fetch(hhx_bam *b, int32_t *id1, int32_t *pos1, int32_t *id2, int32_t *pos2);   /* host copies of the last batch */
int hhx_bam_close(hhx_bam *b);

/* ------------------------------------------------------------------ f4: `haphic plot` contact map
 * HapHiC_plot.py parse_pairs :153-202 / parse_bam :205-245: contact_matrix[bin(ref, pos), bin(mref, mpos)] += 1 per read
 * pair whose two contigs are in ctg_set, with convert_group_bin_id :155-168 as the position -> total scaffold bin lookup.
 * The reference's dicts, flattened (haphic_amd/plot.py does this from ctg_dict / ctg_aln_dict / group_to_total_bin_dict):
 *   in_set[c]                       contig c is in ctg_set (:145-148)
 *   aln_ptr[c] .. aln_ptr[c + 1]    slots of the contig's alignment bins 0, 1, ... (slot = aln_ptr[c] + (pos - 1) // bin_size)
 *   list_ptr[slot] .. [slot + 1]    the closed ranges ctg_aln_dict[ctg][bin] lists, in list order; an empty list = no such key
 *   seg_lo/seg_hi/seg_bin[k]        range on the raw contig (1-based, closed) and group_to_total_bin_dict[ctg_dict[ctg][range]],
 *                                   -1 when the scaffold is not in group_list (the pair is skipped, :161-162)
 * hhx_contact_map_push adds a batch (ids < 0 are skipped: unknown names, filtered BAM records, unmapped mates;
 * pos_offset is added to every position: 0 for .pairs text, 1 for BAM's 0-based reference_start :232 :236).
 * *bad = -1, or 2 * k + side of the first pair k whose position has no alignment bin — where the reference raises
 * 'Cannot find alignment position' (:165-168); the counts of that batch are then meaningless, as in the reference.
 * hhx_contact_map_fetch: the n_total_bins x n_total_bins int64 matrix, row major (numpy dtype=int, :144). */
typedef struct hhx_contact_map hhx_contact_map;
int hhx_contact_map_create(int32_t n_ctg, const uint8_t *in_set, const int64_t *aln_ptr, const int32_t *list_ptr, int64_t n_list,
                           const int32_t *seg_lo, const int32_t *seg_hi, const int32_t *seg_bin, int32_t bin_size, int32_t n_total_bins,
                           hhx_contact_map **out);
int hhx_contact_map_push(hhx_contact_map *m, int64_t n_pairs, const int32_t *id1, const int32_t *pos1, const int32_t *id2, const int32_t *pos2,
                         int on_device, int32_t pos_offset, int64_t *bad);
int hhx_contact_map_fetch(hhx_contact_map *m, int64_t *cells_host);
int hhx_contact_map_device(hhx_contact_map *m, void **cells_dev_i64, int32_t *n_total_bins);
int hhx_contact_map_destroy(hhx_contact_map *m);

/* ------------------------------------------------------------------ f4: `haphic plot` normalisation and vmax
 * HapHiC_plot.py bnewt :291-404 (Knight-Ruiz balancing, float64, tol 1e-6, delta 0.1, Delta 3, g 0.9, etamax 0.1, at most 1000
 * outer / 10000 inner steps) and normalize_matrix :407-504, on the n x n scaffold-bin matrix (haphic_amd/csrc/hhx_plotnorm.hip).
 * hhx_plotnorm_create takes the host matrix (int64, row major) into HBM as int32 counts and reports its max, min and whether it
 *   is symmetric; a negative count or one >= 2^31 leaves a handle every later call refuses.  A[i][j] = (double)count + 0.00001 (:420).
 * hhx_plotnorm_set_blocks: the scaffold blocks [lo[g], hi[g]) — ascending, disjoint, the bins outside belong to no block.
 * hhx_plotnorm_balance: bnewt on every block, then on the whole matrix; entry g < n_blocks of outer / mvp / status is block g,
 *   entry n_blocks the whole matrix: outer steps, matrix-vector products (MVP :388), status 0 = converged, 1 = a cap was reached
 *   (the reference raises 'Unable to converge'), 2 = no step to the bound exists (the reference's min() of an empty list).  The
 *   call returns at the first status != 0.  Same bits on every run: all reductions have a fixed order.
 * hhx_plotnorm_fetch_x: x of the whole matrix and the blocks' x, each at its bins (0.0 outside the blocks); either may be null.
 * hhx_plotnorm_apply: the float64 n x n result to the host: (x[i] * A[i][j]) * x[j] with the block's x inside a block and the
 *   whole matrix's x elsewhere (:431 :437 :446), exactly 0.0 where the count is 0 (:418 :454).
 * hhx_plotnorm_median: the two middle values (as 64-bit patterns; equal when the count is odd) of the off-diagonal cells of
 *   all blocks (:447-450 / :482-485) and their number; kr != 0: the doubles (x[i] * A[i][j]) * x[j] BEFORE the zeros are restored,
 *   kr == 0: the integer counts.  np.median is the mean of the two.
 * hhx_plotnorm_matvec: out = A[lo:hi, lo:hi] @ v with host vectors (the mat-vec kernel alone).
 * hhx_select_middle_u64: the same selection over `count` host values (unsigned order; non-negative doubles order like their bits). */
typedef struct hhx_plotnorm hhx_plotnorm;
int hhx_plotnorm_create(const int64_t *matrix, int32_t n, hhx_plotnorm **out, int64_t *max, int64_t *min, int32_t *symmetric);
int hhx_plotnorm_set_blocks(hhx_plotnorm *h, int32_t n_blocks, const int32_t *lo, const int32_t *hi);
int hhx_plotnorm_balance(hhx_plotnorm *h, int32_t *outer, int64_t *mvp, int32_t *status);
int hhx_plotnorm_fetch_x(hhx_plotnorm *h, double *x_all, double *x_blocks);
int hhx_plotnorm_apply(hhx_plotnorm *h, double *out_host);
int hhx_plotnorm_median(hhx_plotnorm *h, int32_t kr, int64_t *count, uint64_t *lo, uint64_t *hi);
int hhx_plotnorm_matvec(hhx_plotnorm *h, int32_t lo, int32_t hi, const double *v, double *out);
int hhx_plotnorm_destroy(hhx_plotnorm *h);
int hhx_select_middle_u64(const uint64_t *vals, int64_t count, uint64_t *lo, uint64_t *hi);

/* HT_link_dict's insertion order (update_HT_link_dict :404-416): first[4 * k + q] = stream position (among the pairs that
 * entered full_link_dict) of the first read pair of contig pair k (dict order of hhx_ingest_fetch) in quadrant
 * q = [HH, HT, TH, TT], INT64_MAX if the quadrant is empty.  Needs hhx_ingest_keep_pairs. */
int hhx_ingest_fetch_ht_order(hhx_ingest *h, int64_t *first);
/* ctg_pair_to_frag :1731-1733 (split contigs + --remove_allelic_links): every distinct oriented fragment pair the
 * stream produced, whatever its flank / Nx status.  Request before the first push; fetch after finalize (call with
 * NULL arrays for the size). */
int hhx_ingest_keep_frag_pairs(hhx_ingest *h, int on);
int hhx_ingest_fetch_frag_pairs(hhx_ingest *h, int64_t *n_pairs, int32_t *frag_i, int32_t *frag_j);

/* --remove_allelic_links on the device tables (remove_allelic_HiC_links :474-692, haphic_amd/csrc/hhx_allelic.hip): stage 1 and the drop of
 * the verdict on a finalized handle, stage 2 (hhx_allelic_nonmax, below them) on host arrays; only the allele groups (networkx cliques) are
 * host code.  The two hhx_ingest_ entries take a finalized handle; a return value of HHX_UNSUPPORTED (hhx_last_error() says why) means "not served here, take the reference's loop" and
 * leaves the handle untouched.
 *
 * hhx_ingest_concordance: record_coord_pairs :454-465 + cal_concordance_ratio :419-428 as integers.  For every full_link_dict key, in dict
 * insertion order (the order of hhx_ingest_fetch; host arrays [n_full_keys]):
 *   m    = min(count, max_read_pairs);
 *   diag = the modal count of floor((y - x) / w) over the key's first m read pairs in STREAM order (across pushes),
 *   anti = the modal count of (y + x) / w over the same pairs, w = min(len_i, len_j) / nwindows (integer division, :421),
 * x, y the oriented 1-based contig coordinates of the kept read pairs (hhx_ingest_keep_pairs).  The ratio of :428 is
 * max(diag / m, anti / m) in float64 on the host: the same two IEEE divisions, so no float leaves the device.  Keys with
 * m < min(min_read_pairs, max_read_pairs) are not evaluated (:589) and get diag = anti = 0.  One wavefront per key: up to 256 pairs an
 * all-pairs equality count out of LDS, above that a sort in LDS and the longest run.  max_read_pairs is served up to 4096 (the list one
 * wavefront sorts in 32 KB of LDS); beyond that, and when a contig is shorter than nwindows (w = 0: the reference raises), HHX_UNSUPPORTED.
 * The grouped read pairs stay in HBM; the call only reads the kept pairs (a queued paired_links.clm may be reading them too).
 *
 * hhx_ingest_drop_links: update_link_dicts :488-509 for a whole verdict at once, and the isolated-fragment pass :678-692.
 *   full_drop [n_full_keys] (host): non-zero = the key leaves full_link_dict;  in_set [n_frag] (host): the fragment is in filtered_frags.
 * A flank_link_dict key leaves when the contig pair of its two fragments was dropped and both fragments are in in_set — with split contigs
 * through the fragment -> contig map (what ctg_pair_to_frag :1731 encodes; bins of one contig are never affected), else it is the same key.
 * Outputs (host, each may be null): the sizes of the two dicts afterwards; flank_dropped [n_flank_keys before the call], in dict order;
 * remaining [n_frag]: the fragment is in in_set and occurs in a surviving flank key whose other fragment is in in_set too (:680-683);
 * first_row [n_frag]: 2 * (dict position of the first such key) + (1 if the fragment is its second name), -1 if none — sorting by it gives
 * the order in which :680-683 meets the fragments.  The rows say "not in this dict" from then on (first-seen ordinal = UINT64_MAX), so
 * hhx_ingest_fetch, _flank_device (the float64 values, weights included, are carried over), _link_matrix, _write_link_pickle_async, _table_device
 * and the sharded builds see the smaller dicts; frag_links (frag_link_dict) and the HT counts of the surviving keys do not change.  The kept
 * read pairs no longer match the table: hhx_ingest_fetch_pairs / _fetch_ht_order / _fetch_ht_items / _write_clm / _concordance fail afterwards
 * (the reference writes HT_links.pkl and paired_links.clm before :2911).  Waits for the files queued on this handle first. */
#define HHX_UNSUPPORTED 2
int hhx_ingest_concordance(hhx_ingest *h, int64_t max_read_pairs, int64_t min_read_pairs, int64_t nwindows, int32_t *m, int32_t *diag,
                           int32_t *anti);
int hhx_ingest_drop_links(hhx_ingest *h, const uint8_t *full_drop, const uint8_t *in_set, int64_t *n_full_left, int64_t *n_flank_left,
                          uint8_t *flank_dropped, uint8_t *remaining, int64_t *first_row);
/* Stage 2 of the same function, the links between non-maximum matches :621-667, on plain host arrays (no handle; like hhx_group_link_sums).
 *   ki, kj, kcnt [n_keys]: the keys of full_link_dict that survive stage 1, in dict order, as contig ids and counts;
 *   gptr [n_groups + 1], gmem: the allele groups as contig ids, group index = rank of the group under the reference's comparison of name tuples
 *   (tuple(sorted([group_1, group_2])) :644), members in tuple order (position = .index()).
 * A key is a candidate when both contigs are in a group (:639); it yields one combination per (group of ctg_1) x (group of ctg_2); the matrix of
 * a pair of groups (:552-568, degree = the longer group) is filled from the combinations of that pair, and a combination is a mismatch when the
 * matrix has more than one non-zero cell and linear_sum_assignment(-matrix)[1][index_1] != index_2 (:661).  nonmax [n_keys]: 1 = some
 * combination of the key mismatches.  counters [3]: candidates, distinct group pairs, pairs whose matrix has more than one non-zero cell.
 * *assert_failed = 1: an `assert` of :652-659 would fail for some combination; nonmax is then unspecified.  The assignments are scipy's own,
 * ties included: the solver restates scipy 1.15's shortest-augmenting-path method step by step in 64-bit integers (haphic_amd/allelic.py
 * lsap_small is the same in Python).  One sort of the combinations by group pair, then one lane per pair with its matrix in LDS; groups of up
 * to 8 contigs are served, a longer one returns HHX_UNSUPPORTED.  The passes are grid-stride; the environment variable HHX_NONMAX_GRID (read at
 * every launch) caps their workgroups.
 *
 * hhx_lsap_small: that solver alone on n square problems: cost [n][d][d] int64 row-major (minimised; |sums of d costs| below 2^62),
 * col4row [n][d], 1 <= d <= 8. */
int hhx_allelic_nonmax(int64_t n_keys, const int32_t *ki, const int32_t *kj, const int64_t *kcnt, int32_t n_ctg, int32_t n_groups,
                       const int64_t *gptr, const int32_t *gmem, uint8_t *nonmax, int64_t *counters, int32_t *assert_failed);
int hhx_lsap_small(int64_t n, int32_t d, const int64_t *cost, int32_t *col4row);

/* ---------------------------------------------------------------- output_statistics :2279-2478: the per-contig group statistics
 * (haphic_amd/csrc/hhx_groupstats.hip; parse_link_dict :2252-2268, sorted :2365, cal_link_density :2271-2276, sum :2376).  One "set" is one
 * group assignment (one inflation): group [n_sets][n_ctg] (host; -1 = 'ungrouped'), n_groups [n_sets], group_re = the sets' group_RE_dict
 * values one set after the other (sum of n_groups entries), ctg_re [n_ctg].  Every key (ctg_i, ctg_j) of full_link_dict contributes
 * (ctg_i, group[ctg_j], links, pos = 2k) and (ctg_j, group[ctg_i], links, pos = 2k + 1), k its dict position; a partner group of -1 is
 * skipped.  The cells of a contig are its distinct groups with sum (int64, exact) and first (smallest pos), ordered by sum descending, then
 * first ascending: the order of the reference's stable sorted(..., reverse=True).  Outputs (host, [n_sets][n_ctg]):
 *   n_cells    number of cells (0: the contig is not in ctg_group_link_dict; max_group is -1 then)
 *   max_links, max_group   the first cell
 *   other_sum  the float64 sum of links / den over the other cells, den = group_re[g] when g is the contig's own group, else
 *              group_re[g] + ctg_re - 1, the quotients added one by one in that order from 0.0.  sum_mode 0: the plain sum (CPython <= 3.11);
 *              1: Neumaier's compensated sum with the final "add the compensation if it is non-zero and finite" of CPython >= 3.12's sum().
 * The sums and denominators are converted to float64 before the division, which is Python's int / int while both stay below 2^53.  The last
 * divisions of :2372-2381 (max_links / den, other_sum / (n_groups - 1), their ratio) are elementwise and left to the caller.
 * The table is turned into a symmetric adjacency by contig once per call; one workgroup per (contig, set) accumulates the cells in LDS
 * (hhx_tune "groupstats_lds_slots"), a contig with more distinct groups than slots is redone on a per-workgroup table in HBM.
 * hhx_ingest_group_stats works on the contig-pair table of a finalized handle (the rows of hhx_ingest_table_device(h, 0, ...); a row whose
 * full ordinal is UINT64_MAX is no key, e.g. after hhx_ingest_drop_links; pos = 2 * ordinal + side): nothing of the table crosses PCIe, the
 * handle is only read.  hhx_group_stats takes the keys as arrays in dict order (host, or device with on_device), like hhx_group_link_sums.
 * HHX_UNSUPPORTED (hhx_last_error() says why): a sum_mode other than 0 / 1, n_ctg * n_sets of 2^31 and more. */
int hhx_ingest_group_stats(hhx_ingest *h, int32_t n_sets, const int32_t *group_host, const int32_t *n_groups, const int64_t *group_re_host,
                           const int64_t *ctg_re_host, int sum_mode, int32_t *n_cells, int64_t *max_links, int32_t *max_group,
                           double *other_sum);
int hhx_group_stats(int64_t n_keys, const int32_t *frag_i, const int32_t *frag_j, const int64_t *links, int on_device, int32_t n_ctg,
                    int32_t n_sets, const int32_t *group_host, const int32_t *n_groups, const int64_t *group_re_host,
                    const int64_t *ctg_re_host, int sum_mode, int32_t *n_cells, int64_t *max_links, int32_t *max_group, double *other_sum);
int hhx_ingest_destroy(hhx_ingest *h);

/* The rescue and reassignment rounds of `haphic reassign` and the group-pair sums of its agglomerative step (HapHiC_reassign.py run_reassignment
 * :266-427, agglomerative_hierarchical_clustering :494-508; haphic_amd/csrc/hhx_reassign.hip).  The handle keeps in HBM: the keys of
 * full_link_dict in dict order, their symmetric adjacency by contig, and per (contig, group) cell `sum` (int64) and `stamp` (the cell's position in
 * the reference's inner dict: 2 * key + side of its first contribution as hhx_group_link_sums defines it, or 2 * n_keys + the number of the move
 * that created it; UINT64_MAX = no cell).  hhx_reassign_create builds them from the keys and the group of every contig (-1 = 'ungrouped');
 * hhx_reassign_cells copies the two tables out as hhx_group_link_sums returns them (first == -1: no cell).
 * hhx_reassign_round is one call of run_reassignment.  group [n_ctg] and group_re [n_groups] (group_RE_dict's values) are uploaded from the
 * caller's arrays at the start of every call and returned at the end; the cells live across calls.  ctg_re [n_ctg] = RE_site_dict, order [n_order]
 * = the contigs of sorted_ctg_list, flags [n_ctg]: bit 0 = the RE filter :335 is passed, bit 1 = short enough to be reassigned :415; dismissed
 * [n_groups] (or NULL) = the groups :304-324 dismisses: their contigs become -1, every contig's links to them 0.  Each contig is judged against the
 * state all earlier contigs of the call left: the non-zero cells ordered by (sum descending, stamp ascending), the filters :335-368 in their order
 * (the ambiguity filter only when is_rescue_round is 0), the densities of all cells after the first added one by one in that order (sum_mode as
 * for hhx_group_stats), divided by n_groups - 1 or, with gfa, by their count; 1000000000 when the sum is 0; the verdicts :392-424.  A move changes
 * group, group_re of the former and the new group, and the two cells of every neighbour.  counts[4] = consistent, rescued, reassigned, not
 * rescued; *launches (may be NULL) = the launch pairs the round took.  A round is a chain of (evaluate a window of the order, commit its first
 * mover) launch pairs in stream order: about n_order / window + movers of them; hhx_tune "reassign_window" bounds the window.  Cells of value 0
 * are not told apart from absent ones, which is the reference's result while min_links >= 1 (anything below is refused).  Sums and RE totals are
 * taken to stay below 2^53.
 * hhx_reassign_pair_sums: for every key in dict order whose two contigs are both in member [n_ctg], both have a group in group_of_ctg (-1 = none)
 * and the groups differ, the links are added to cell (smaller id, larger id) of sums [n_groups][n_groups], and first holds the dict position of
 * the first such key (-1 = none).
 * HHX_UNSUPPORTED (hhx_last_error() says why): n_ctg * n_groups * 16 bytes (the two tables) beyond half of the device's memory; a sum_mode other
 * than 0 / 1. */
typedef struct hhx_reassign hhx_reassign;
int hhx_reassign_create(int64_t n_keys, const int32_t *frag_i, const int32_t *frag_j, const int64_t *links, int32_t n_ctg,
                        const int32_t *group_host, int32_t n_groups, hhx_reassign **out);
int hhx_reassign_cells(hhx_reassign *h, int64_t *sums_host, int64_t *first_host);
int hhx_reassign_round(hhx_reassign *h, int32_t *group_host, int64_t *group_re_host, const int64_t *ctg_re_host, int32_t n_order,
                       const int32_t *order_host, const uint8_t *flags_host, const uint8_t *dismissed_host, double min_links,
                       double min_link_density, double min_density_ratio, double ambiguous_cutoff, int is_rescue_round, int gfa,
                       int sum_mode, int64_t *counts, int64_t *launches);
int hhx_reassign_pair_sums(hhx_reassign *h, const uint8_t *member_host, const int32_t *group_of_ctg_host, int32_t n_groups, int64_t *sums_host,
                           int64_t *first_host);
int hhx_reassign_destroy(hhx_reassign *h);
/* hhx_reassign_create_from_pickle: the handle hhx_reassign_create makes, from the ids and values of an open hhx_pickle (declared below) where they
 * lie in HBM: device-to-device copies, no key crosses the bus.  The ids are the pickle's name ids; n_ctg >= its name count (the contigs no key names
 * follow the names; group_host [n_ctg]).  One pass over the keys first decides what the mirror of parse_link_dict decides on host arrays
 * (haphic_amd/reassign.py): *refused = an OR of the flags below when a key names one contig twice, a value is a float, a value is negative, or twice
 * the total of the values reaches 2^53 (the low and the high 32 bits of the values are added apart and put together in 128 bits, so the pass's own
 * sum cannot wrap), or the table holds 2^31 keys and more.  Then *out = NULL, the return value is 0 and hhx_last_error() holds the reason: the
 * caller takes the host path.  HHX_UNSUPPORTED as for hhx_reassign_create: the cells beyond half of the device's memory.
 * The pass is grid-stride; hhx_tune "reassign_check_grid" caps its workgroups. */
#define HHX_REFUSED_SELF_KEY 1
#define HHX_REFUSED_FLOAT 2
#define HHX_REFUSED_NEGATIVE 4
#define HHX_REFUSED_TOTAL 8
#define HHX_REFUSED_KEYS 16
struct hhx_pickle;
int hhx_reassign_create_from_pickle(struct hhx_pickle *p, int32_t n_ctg, const int32_t *group_host, int32_t n_groups, int *refused, hhx_reassign **out);

/* Multi-GPU exchange step (ingest).  The aggregated table of a finalized handle, device
 * SoA in no particular order: key = (i << 29) | j, first-seen global ordinals of the key in
 * full_link_dict / flank_link_dict (UINT64_MAX = never), HT counts [n][4], flank count.
 * which = 0: contig-pair table, 1: fragment-pair flank table (the same table unless contigs are split).
 * hhx_ingest_push_table feeds such rows (e.g. the all-gathered tables of every rank) into another handle;
 * its finalize merges them: counts add, ordinals take the minimum — exactly the reference loop run over
 * the concatenated stream. */
int hhx_ingest_table_device(hhx_ingest *h, int which, int64_t *n_rows, void **dev_key_u64, void **dev_ord_full_u64,
                            void **dev_ord_flank_u64, void **dev_ht_u32x4, void **dev_flank_u32);
int hhx_ingest_push_table(hhx_ingest *h, int which, int64_t n_rows, const uint64_t *dev_key, const uint64_t *dev_ord_full,
                          const uint64_t *dev_ord_flank, const uint32_t *dev_ht, const uint32_t *dev_flank);


/* ---------------------------------------------------------------- the files run() writes from the S5 containers (:2879-2929)
 * With the link tables held as arrays (haphic_amd/containers.py) the reference's writers have array forms:
 *
 * output_clm :376-392 — paired_links.clm from the read pairs kept in HBM (hhx_ingest_keep_pairs): for every contig pair with at
 * least two read pairs (:385), in full_link_dict order, four lines "{ctg_i}{+|-} {ctg_j}{+|-}\t{2 * links}\t{d d d d ...}\n",
 * the distances of update_clm_dict :395-401 for that orientation ascending, each written twice (:388).  Grouping, sorting and
 * the text are made on the device; contig names = UTF-8 bytes back to back (host), name k = [name_off[k], name_off[k + 1]).
 * Returns the numbers of lines and bytes written.  Fails (and leaves a partial file) if a read position lies beyond its contig. */
int hhx_ingest_write_clm(hhx_ingest *h, const char *path, const uint8_t *names_blob, const int64_t *name_off, int64_t *n_lines,
                         int64_t *n_bytes);
/* HT_link_dict (update_HT_link_dict :404-416) as items in dict insertion order, sorted on the device: item t = the t-th (contig
 * pair, quadrant) entry to enter the dict, i.e. ordered by the stream position of its first read pair (hhx_ingest_fetch_ht_order);
 * name_i / name_j = 2 * contig id + (1 if that end is '_T', 0 for '_H'), count = its links.  *n_items is always set; the arrays
 * (host, [*n_items] from a first call with null arrays) are optional.  Needs hhx_ingest_keep_pairs. */
int hhx_ingest_fetch_ht_items(hhx_ingest *h, int64_t *n_items, int32_t *name_i, int32_t *name_j, int64_t *count);
/* the float64 values of the flank table in dict order (host buffer [n_flank_keys]): the counts, or what hhx_link_weights
 * (on_device, over hhx_ingest_flank_device's arrays) left there — normalize_by_nlinks :718-724 on the resident table */
int hhx_ingest_fetch_flank_values(hhx_ingest *h, double *value);
/* output_pickle :710-715 for a link dict given as arrays — full_links.pkl, HT_links.pkl: a protocol-4 pickle of
 * `collections.defaultdict(int)` {(names[name_i[k]], names[name_j[k]]): count[k]}, keys in array order (= dict insertion order),
 * written by host code without a Python object per key; names as for hhx_ingest_write_clm.  pickle.load gives the dict the
 * reference's loops :1605-1615 build.  All pointers host. */
int hhx_write_link_pickle(const char *path, int64_t n_keys, const int32_t *name_i, const int32_t *name_j, const int64_t *count,
                          int32_t n_names, const uint8_t *names_blob, const int64_t *name_off, int64_t *n_bytes);


/* ---------------------------------------------------------------- the same files, off the caller's critical path
 * run() :2879 / :2888 / :2929 writes HT_links.pkl, paired_links.clm and full_links.pkl between its seams and reads none of them again
 * (the next readers are `haphic sort` / `haphic reassign`, other processes).  The *_async entry points check their arguments, refuse
 * what the writer would refuse (a read position beyond its contig's end) and open the file on the CALLER's thread, then queue the work
 * on a host thread owned by the library — two lanes (the byte sinks below; everything else), each running its jobs in submission order on a
 * non-blocking stream of its own with a memory-pool arena of its own, so the device half of a job (grouping / sorting / formatting, hhx_ingest_write_clm; ordering the HT items,
 * hhx_ingest_fetch_ht_items) overlaps the caller's next kernels — and return at once.  hhx_files_join waits for every queued file and
 * returns non-zero with the first failure as hhx_last_error() (*n_failed = how many files failed; the failures are forgotten after the
 * call); hhx_ingest_destroy waits for the jobs that read its handle.  A process that exits without hhx_files_join still gets its
 * files: the library's destructor works the queue off.
 *
 * hhx_ingest_write_clm_async: output_clm :376-392.  drop_pairs_after != 0: the kept read pairs (16 B per pair of HBM) are released when
 * the file is complete — afterwards hhx_ingest_fetch_pairs / _ht_order / _ht_items / _write_clm on this handle fail (with that message).
 * hhx_ingest_write_link_pickle_async: output_pickle :710-715 of a table of the handle — which = 0 full_link_dict (names = contigs),
 * 1 HT_link_dict (names = [c0 + "_H", c0 + "_T", c1 + "_H", ...], items ordered on the device), 2 flank_link_dict with its integer counts
 * (names = fragments); the writer thread fetches the items into host memory of its own.
 * hhx_write_link_pickle_async: hhx_write_link_pickle of arrays the CALLER owns: name_i / name_j / count must stay valid and unchanged until
 * hhx_files_join returns (names_blob / name_off are copied). */
int hhx_ingest_write_clm_async(hhx_ingest *h, const char *path, const uint8_t *names_blob, const int64_t *name_off, int drop_pairs_after);
int hhx_ingest_write_link_pickle_async(hhx_ingest *h, int which, const char *path, int32_t n_names, const uint8_t *names_blob,
                                       const int64_t *name_off);
int hhx_write_link_pickle_async(const char *path, int64_t n_keys, const int32_t *name_i, const int32_t *name_j, const int64_t *count,
                                int32_t n_names, const uint8_t *names_blob, const int64_t *name_off);
/* alignments.bed (pairs_generator* :1549-1557: two records per read pair, written inside the generator's loop, read by nothing in run()), deferred:
 * a byte sink is a file fed from DEVICE memory through the same writer thread.  The producer reserves room in the sink's ring of HBM slabs
 * (hhx_byte_sink_reserve: returns at once while fewer than hbm_budget_bytes are waiting to be written — <= 0: a quarter of the device, or
 * HHX_BED_HBM_GB — and holds the caller at the writer's pace beyond that), launches the kernel that fills it on its own stream, and commits
 * (hhx_byte_sink_commit: the range is queued; the writer waits for the kernel through an event).  expected_bytes (0: unknown) sizes the slabs.
 * hhx_pairs_parser_set_bed_sink makes hhx_pairs_parse(want_bed) do exactly that with the BED records of every chunk.  hhx_byte_sink_close
 * queues the close and frees the handle when it has run: the file is complete after hhx_files_join. */
typedef struct hhx_byte_sink hhx_byte_sink;
int hhx_byte_sink_open(const char *path, int64_t hbm_budget_bytes, int64_t expected_bytes, hhx_byte_sink **out);
int hhx_byte_sink_reserve(hhx_byte_sink *sink, int64_t n_bytes, void **dev);
int hhx_byte_sink_commit(hhx_byte_sink *sink, void *dev, int64_t n_bytes);
int hhx_byte_sink_close(hhx_byte_sink *sink, int64_t *n_bytes_pushed);
/* a sink whose bytes start at a file offset known only later (one rank's share of alignments.bed, behind the ranks before it): the file is not
 * truncated, committed ranges stay parked in their slabs until hhx_byte_sink_set_base(base) — when the HBM budget runs out before that, they spill
 * in order to a part file beside the target, copied into place by the set_base job.  Closing it before set_base writes nothing and fails the close. */
int hhx_byte_sink_open_deferred(const char *path, int64_t hbm_budget_bytes, int64_t expected_bytes, hhx_byte_sink **out);
int hhx_byte_sink_set_base(hhx_byte_sink *sink, int64_t base);
int hhx_pairs_parser_set_bed_sink(hhx_pairs_parser *p, hhx_byte_sink *sink);
/* paired_links.clm split by group for `haphic reassign`: split_clm_file, scripts/HapHiC_reassign.py:581-622.  Per line (text mode, universal
 * newlines: '\n', "\r\n" and a lone '\r' end a line, which is written with '\n'; a last line without a break keeps none): cols = line.split();
 * the last character of cols[0] and of cols[1] is dropped; the line goes verbatim to the file of the group both names belong to, when both are
 * in the table and in the same group (group_of_name[k] in [0, n_groups), -1: in no group).  Every group's file (paths_blob / path_off, one path
 * per group) is created, possibly empty; lines keep file order inside a file; at most n_groups descriptors are open, as in the reference.
 * hhx_clm_split_push takes ANY byte range of the file, in order: a cut may fall anywhere (inside a token, between '\r' and '\n', inside a line
 * of megabytes, which is never held whole).  Only the head of a line whose first two tokens are not complete yet is buffered (at most 64 KB,
 * a clear failure beyond).  hhx_clm_split_file pushes the whole file as raw chunks of chunk_bytes from pinned read-ahead buffers.
 * The first line with fewer than two tokens fails the call with "IndexError: list index out of range" in hhx_last_error(), as :617 raises;
 * a line still open at hhx_clm_split_finish counts too unless it has no bytes.  hhx_clm_split_finish flushes the open line and waits for the
 * writer lanes: the files are complete and closed on return (bytes_per_group[n_groups], may be NULL).  Whitespace is the ASCII subset of
 * str.split()'s, bytes >= 0x80 are name bytes (as for hhx_pairs_parse).
 * hhx_clm_split_stats: values[HHX_CLM_SPLIT_N_STATS] = lines parsed, lines kept, heads carried to the next push, "\r" | "\n" seams joined,
 * continuation segments of an open line, gather tiles that held more than one line, lines that spanned more than one gather tile. */
#define HHX_CLM_SPLIT_N_STATS 7
typedef struct hhx_clm_split hhx_clm_split;
int hhx_clm_split_create(int32_t n_names, const uint8_t *names_blob, const int64_t *name_off, const int32_t *group_of_name, int32_t n_groups,
                         const uint8_t *paths_blob, const int64_t *path_off, hhx_clm_split **out);
int hhx_clm_split_push(hhx_clm_split *s, const uint8_t *text, int64_t n_bytes, int on_device);
int hhx_clm_split_file(hhx_clm_split *s, const char *clm_path, int64_t chunk_bytes, int n_threads);
int hhx_clm_split_finish(hhx_clm_split *s, int64_t *n_lines, int64_t *n_kept, int64_t *bytes_per_group);
int hhx_clm_split_stats(hhx_clm_split *s, int64_t *values);
int hhx_clm_split_destroy(hhx_clm_split *s);
int hhx_files_pending(int64_t *n_pending, int64_t *n_done);
int hhx_files_join(int64_t *n_failed);

/* ---------------------------------------------------------------- full_links.pkl / HT_links.pkl back into arrays (haphic_amd/csrc/hhx_pickleread.hip)
 * HapHiC_reassign.py parse_pickle :38-50 is `pickle.load(f)`: a defaultdict(int) {(name, name): value} of every key, which the next step flattens
 * again.  hhx_pickle_open reads the file into HBM (pinned read-ahead of hhx_text_reader_open_raw), finds the opcode boundaries on the device, validates
 * the stream token by token and leaves, in dict insertion order: name_i / name_j [n_keys] (int32 ids), the 64 bits of every value (two's complement of
 * an int, IEEE-754 of a float) with is_float [n_keys], and the distinct names — compared as bytes, numbered in order of first appearance, i before j,
 * key by key — as names_blob + name_off [n_names + 1].  Accepted: protocol 4 or 5; an optional FRAME; the construction of
 * collections.defaultdict(builtins.int) as the pickler and hhx_write_link_pickle spell it; then any interleaving of FRAME, MARK, SETITEMS, SETITEM and
 * MEMOIZE that a sequential reader accepts around the items *name, name, TUPLE2, value*; STOP as the last byte.  name = SHORT_BINUNICODE, or BINGET /
 * LONG_BINGET of a slot a name literal was memoised into; value = BININT1, BININT2, BININT, LONG1 of at most 8 bytes, BINFLOAT.  Everything else — another
 * header or protocol, any other opcode (BINUNICODE of a name of 256 bytes and more, LONG1 of 9 bytes and more, TUPLE3, NEWTRUE, NONE ...), a memo
 * reference to a tuple or to one of the header's slots, a MEMOIZE of anything but a name literal or a key, a key written twice, frames that do not
 * tile the file, a file that ends early, bytes after STOP, a file beyond half of the device's memory — returns HHX_PICKLE_NOT_OURS with the reason in
 * hhx_last_error() and *out = NULL: the caller runs pickle.load, so that Python's own answer is what the user sees.  Any other non-zero return is a
 * failure (I/O, memory).  The boundary search works on chunks of hhx_tune "pkl_chunk" bytes.  hhx_pickle_fetch copies into host arrays (any may be
 * NULL); hhx_pickle_free(NULL) is fine. */
#define HHX_PICKLE_NOT_OURS 2
typedef struct hhx_pickle hhx_pickle;
int hhx_pickle_open(const char *path, hhx_pickle **out);
int hhx_pickle_sizes(hhx_pickle *p, int64_t *n_keys, int32_t *n_names, int64_t *names_bytes, int *any_float);
int hhx_pickle_fetch(hhx_pickle *p, int32_t *name_i, int32_t *name_j, int64_t *value_bits, uint8_t *is_float, uint8_t *names_blob, int64_t *name_off);
int hhx_pickle_free(hhx_pickle *p);
/* One group's H/T links from the open table: HapHiC_sort.py get_sub_HT_dict :117-143, which run() :898-901 / :912-920 calls per group on the dict
 * pickle.load built from HT_links.pkl.  For ctgs in the order parse_group returns them (n = n_ctg distinct names, 2 <= n < 2^30) the caller passes
 * slot [n_names] = 2 * position + suffix (0: '_H', 1: '_T') for the names ctg + '_H' / ctg + '_T' the file holds (whole names: nothing is stripped from a
 * name of the file) and -1 for every other name, and rank [n] = the place of every position among the sorted names (Python's string order; a
 * permutation).  A key (x, y): v of the table is kept exactly when x and y are slotted names of two different contigs c1, c2, c1 < c2 as strings
 * (rank), and v != 0; keys written the other way round, keys between the two ends of one contig and zero values never are.  A kept key becomes
 * (index[x], index[y]): v with HT_index_dict's closed form — lo, hi = sorted(ctgs[:2]): lo_H = 0, hi_H = 1, hi_T = 2, lo_T = 3; ctgs[k]_H = 2 k,
 * ctgs[k]_T = 2 k + 1 from k = 2 on — and the edges are left in the handle in the reference's insertion order: ascending in
 * ((a * n + b) << 2) | (2 * [x ends in T] + [y ends in T]), a < b the positions of the two contigs.  On the device: a streaming pass over the ids of
 * the table (both ends are first tested against a bitmap of the slotted names in LDS: hhx_tune "heads_bitmap") that counts the survivors of every
 * wavefront's range, the same pass again to write them (ballot and prefix inside the wavefront, no counter shared between wavefronts), and a stable
 * radix sort on the 2 * ceil(log2 n) + 2 bits of that order key; nothing of slot / rank is kept between calls.  *n_edges: the edges found;
 * hhx_pickle_group_heads_fetch copies the last call's ei / ej (int32 indices) and w (int64 values) into host arrays (any may be NULL).  A table with
 * float values, n_ctg outside 2 .. 2^30 - 1, a slot outside -1 .. 2 n - 1 and a rank that is no permutation are errors. */
int hhx_pickle_group_heads(hhx_pickle *p, int32_t n_ctg, const int32_t *slot, const int32_t *rank, int64_t *n_edges);
int hhx_pickle_group_heads_fetch(hhx_pickle *p, int32_t *ei, int32_t *ej, int64_t *w);

/* ---------------------------------------------------------------- assembly correction (--correct_nrounds), haphic_amd/csrc/hhx_correct.hip
 * Pass one — parse_pairs_for_correction :1300-1344 / parse_bam_for_correction :1362-1398.  hhx_correct_create: contig c (fa_dict order, ctg_len
 * host) owns ctg_len[c] // resolution + 1 bins (:1311) of one flat int32 coverage array.  Positions and coverage are int32 as in the reference
 * (array('i') :1308, ndarray int32 :1311): a contig of 2^31 - 1 bp or more is refused.  hhx_correct_push takes the four arrays the tokeniser
 * (hhx_pairs_parser_arrays) and the BAM decoder (hhx_bam_next) leave on the device (or host arrays, on_device = 0): a record is kept iff
 * id1 == id2 >= 0 (:1327-1332; BAM records that fail `flag.read1 && refid == mrefid` :1376 carry id -2 or two different ids); lo, hi = sorted(pos, mpos)
 * :1337; coverage of bins lo // res .. hi // res += 1, clipped at the contig's last bin as the numpy slice :1341 is; (lo, hi) joins the contig's
 * position list :1342 in file order.  A negative position fails the push.  hhx_correct_finalize: the position lists grouped by contig (stable),
 * the coverage summed; *n_kept = kept records.
 * The table: segment s = (first bin in the flat array, bins, length, pairs [pair_off[s], pair_off[s + 1])) — the contigs of the FASTA after
 * finalize, the children of the broken contigs after hhx_correct_break.  hhx_correct_fetch_*: host copies (any pointer of _segments may be null);
 * coverage = the whole flat array [n_bins of hhx_correct_shape], pairs = lo, hi interleaved [2 * n_pairs] in segment order.
 * hhx_correct_detect — detect_break_points :943-1014 over every segment, arithmetic as the kernel's comment spells it out (numpy median, float64
 * cut-offs): n_bp[s] break points in segment s (0: none) at coverage bp_cov[s] (0: the zero-coverage case, possibly several points; else one point),
 * *n_total their sum; hhx_correct_fetch_break_points: their BINS (position = bin * resolution), segment order, ascending inside a segment.
 * hhx_correct_break — the per-pair half of break_and_update_ctgs :1063-1113 and the coverage slices :1153 :1178 for the n_broken segments seg[]
 * (ascending) with break POSITIONS bp_pos[bp_off[b] .. bp_off[b + 1]) (ascending multiples of the resolution inside the contig) and zero[b] bit 0 =
 * the zero-coverage case (:1068), bit 1 = the contig is a piece that does not start its original contig (pos_shift :1050 then files the pairs of every child
 * but the last under a name nothing reads again: they are dropped, as the reference loses them): pairs meeting [bp, bp + res] are dropped and their coverage taken back (non-zero case), the others move to the
 * child holding both ends or are dropped when the ends part; child k of a contig is a view [start // res, point // res) of its parent's bins, the
 * last child runs to the parent's last bin; the new table holds the children alone, in (parent, child) order (:1192-1197). */
typedef struct hhx_correct hhx_correct;
int hhx_correct_create(int32_t n_ctg, const int64_t *ctg_len, int32_t resolution, hhx_correct **out);
int hhx_correct_push(hhx_correct *c, int64_t n, const int32_t *id1, const int32_t *pos1, const int32_t *id2, const int32_t *pos2, int on_device);
int hhx_correct_finalize(hhx_correct *c, int64_t *n_kept);
/* Partial tables (the ranks of a --gpus N job fill one each from their byte range of the file, haphic_amd/ranks.py phase `correct_pass1`).  Until
 * hhx_correct_finalize a table is a coverage difference array [n_bins] (+1 at the first bin of a kept record :1341, -1 behind its last) and the
 * kept records (contig, lo, hi) in push order: difference arrays of disjoint record sets add, record lists concatenate, so absorbing the tables of
 * consecutive pieces of a stream IN ORDER and finalizing gives the table of one pass over the whole stream, bit for bit (coverage, segments, the
 * position lists :1342 in file order).  hhx_correct_export: *resolution, *n_bins, *n_pairs of a table that is not finalized (any may be null), and
 * — where the pointers are not null — its difference array [n_bins] and its records [pair_first, pair_first + pair_count) in push order as
 * pair_ctg [pair_count], pair_lo_hi [2 * pair_count] (lo, hi interleaved), into host arrays or (on_device) device arrays; the table is left as it
 * was.  A large table goes out in pieces: the difference array once, the records a range at a time.  hhx_correct_absorb adds such a piece to c
 * (cov_diff null: records alone; n_pairs 0: the difference array alone; at most 2^31 - 1 records a call): a resolution or bin count other than
 * c's, or a finalized c, is refused before anything is touched; a record no push keeps (contig outside the table, not 0 <= lo <= hi) fails the
 * call and leaves c unfit for hhx_correct_finalize. */
int hhx_correct_export(hhx_correct *c, int32_t *resolution, int64_t *n_bins, int64_t *n_pairs, int32_t *cov_diff, int64_t pair_first,
                       int64_t pair_count, int32_t *pair_ctg, int32_t *pair_lo_hi, int on_device);
int hhx_correct_absorb(hhx_correct *c, int32_t resolution, int64_t n_bins, const int32_t *cov_diff, int64_t n_pairs, const int32_t *pair_ctg,
                       const int32_t *pair_lo_hi, int on_device);
int hhx_correct_shape(hhx_correct *c, int32_t *n_seg, int64_t *n_bins, int64_t *n_pairs);
int hhx_correct_fetch_segments(hhx_correct *c, int64_t *bin_off, int32_t *n_bins, int32_t *len, int64_t *pair_off);
int hhx_correct_fetch_coverage(hhx_correct *c, int32_t *cov);
int hhx_correct_fetch_pairs(hhx_correct *c, int32_t *lo_hi);
int hhx_correct_detect(hhx_correct *c, double median_cov_ratio, double region_len_ratio, int64_t min_region_cutoff, int32_t *n_bp, int32_t *bp_cov,
                       int64_t *n_total);
int hhx_correct_fetch_break_points(hhx_correct *c, int32_t *bp_bin);
int hhx_correct_break(hhx_correct *c, int32_t n_broken, const int32_t *seg, const int64_t *bp_off, const int32_t *bp_pos, const uint8_t *zero);
int hhx_correct_destroy(hhx_correct *c);
/* Pass two — convert_ctg :1405-1411 (and its copies :1447-1453 :1477-1483 :1516-1522) between a front end and hhx_ingest_push: source contig s
 * (the names the tokeniser / BAM decoder was given) owns entries [off[s], off[s + 1]) of (break_pos ascending, new_id): (s, x) becomes
 * (new_id, x - break_pos) of the entry with the largest break_pos <= x; an unbroken contig has the one entry (0, its id in the corrected FASTA); a
 * source without entries, or x below its first entry, becomes id -1 (dropped by the ingest like any name outside fa_dict).  Negative ids pass
 * through.  hhx_remap_apply works in place on one (id, position) column pair on the device, on the library's stream. */
typedef struct hhx_remap hhx_remap;
int hhx_remap_create(int32_t n_src, const int32_t *off, const int32_t *break_pos, const int32_t *new_id, hhx_remap **out);
int hhx_remap_apply(hhx_remap *r, int64_t n, int32_t *dev_id, int32_t *dev_pos);
int hhx_remap_destroy(hhx_remap *r);

/* ---------------------------------------------------------------- `haphic sort`: fast sorting (HapHiC_sort.py fast_sort :470-615)
 * One handle per group holds the dense work of every round on the device (csrc/hhx_sort.hip); the spanning forest and the work on names stay on the host.
 * hhx_sort_graph_create — dict_to_matrix :60-88 of round 1: the dict's keys (index pairs in [0, shape), either orientation, no pair twice) and integer
 *   weights >= 0 become the dense symmetric float32 link matrix; the edge list stays on the device for the whole group, because update :406-435 always
 *   aggregates from old_sub_HT_matrix.  shape: even, at least 4.
 * hhx_sort_graph_density — get_density_graph :158-192: len[shape] float64 (get_HT_len of every index, flank_HT_dict included); L[i][j] = len_i + len_j
 *   (method 0, 'sum'), len_i * len_j (1, 'multiplication') or sqrt(len_i * len_j) (2, 'geometric_mean') in float64, rounded to float32, 1 on the diagonal;
 *   D = S / L in float32.  Method 2 reports in *n_flagged the pairs i < j whose float64 root lies within 2 ulp of a float32 rounding boundary (Python's
 *   (a * b) ** 0.5 may round the other way): hhx_sort_graph_fetch_flagged copies them (i, j interleaved), the caller computes L with ** and hands it
 *   to hhx_sort_graph_patch_len, which redoes D[i][j] = D[j][i] = S / L.
 * hhx_sort_graph_confidence — get_unfiltered_confidence_graph :195-244 on the current edges: out[shape * shape + 1] float64 receives the matrix (0 where
 *   no edge; per edge 0 if its density is 0, 2 if the second largest density incident on either end is 0, else float32(d / second); sister pairs
 *   (pair_a[k], pair_b[k]) get 2 * MAXS if MAXS > 1 else 2) and, in its last element, MAXS — one copy.
 * hhx_sort_graph_drop — remove_shortest_path :456-467: the edges touching a or b (which must be the last two indices) leave the current edge list,
 *   the matrices keep their pitch and lose their last two rows and columns (no copy).
 * hhx_sort_graph_aggregate — the link re-aggregation of update :406-435: map[old index of round 1] = new index or -1; every round-1 edge (a, b, w) with
 *   i = map[a], j = map[b], both >= 0, i != j, i ^ 1 != j adds w to cell (max, min) of an integer accumulator (in LDS while new_shape <= 192 and the
 *   weights sum to less than 2^32, hhx_tune "sort_lds_shape"; with global atomics above).  The handle then holds the new link matrix and the new edge
 *   list (keys (i_1, i_2) with i_1 > i_2 in row-major order, float32 values: hhx_sort_graph_fetch_edges).  *n_over: cells whose sum exceeds 2^24, where
 *   the reference's float32 running sum may round: hhx_sort_graph_fetch_over copies their positions (i_1 * new_shape + i_2, any order), the caller sums
 *   them in the reference's order and hands the values to hhx_sort_graph_patch_cells (ordinal: the edge's position in the list).
 * hhx_sort_graph_fetch_dense: the leading shape x shape block of the link matrix (which = 0) or the density graph (1), row-major float32.
 * hhx_sort_graph_stats: values[HHX_SORT_GRAPH_N_STATS] = re-aggregations through LDS, through global atomics, cells above 2^24 of the last one, flagged
 *   pairs of the last density call.
 * hhx_sort_graph_confidence_device — hhx_sort_graph_confidence without the copy: the matrix stays on the device, *maxs receives MAXS (8 bytes).
 *   hhx_sort_graph_fetch_confidence copies the shape x shape matrix as it is now (filtered, once hhx_sort_graph_forest ran) into out[shape * shape].
 * hhx_sort_graph_forest — fast_sort :567-570 on the matrix of the last confidence call: filter_confidence_graph :247-255 (cells of the current edges
 *   with C <= cutoff become 0, both triangles), then the forest nxtree.maximum_spanning_tree(Graph(C), algorithm='kruskal') returns: the unique maximum
 *   spanning forest under the strict order (weight descending, u ascending, v ascending), u < v, over the non-zero cells of the current edges and the
 *   sister pairs (a pair that is both counts once).  *n_chosen: its edges; *not_paths: 1 when some node has no edge or more than two (fast_sort then
 *   fails its assert :586).  One workgroup on LDS arrays while shape <= 2048 and the edges fit beside the node arrays (12 bytes an edge slot, a power
 *   of two of slots, 48 bytes a node, 160 KiB in all: 4096 edges at shape 2048), hhx_tune "sort_forest_lds"; one launch per phase on HBM arrays above.
 *   shape <= 65535.  hhx_sort_graph_fetch_forest: eu / ev[n_chosen] (u < v) in the order Kruskal emits them, label[shape] = the smallest index of the
 *   node's tree, pos[shape] = the node's position along its path counted from the end with the smaller index (-1 everywhere when not_paths).
 * hhx_sort_graph_forest_stats: values[HHX_SORT_FOREST_N_STATS] = forests through LDS, through HBM, Boruvka rounds and pointer-doubling rounds of the
 *   last one, copies of the confidence matrix to the host (hhx_sort_graph_confidence and hhx_sort_graph_fetch_confidence). */
#define HHX_SORT_GRAPH_N_STATS 4
#define HHX_SORT_FOREST_N_STATS 5
typedef struct hhx_sort_graph hhx_sort_graph;
int hhx_sort_graph_create(int32_t shape, int64_t n_edges, const int32_t *ei, const int32_t *ej, const int64_t *w, hhx_sort_graph **out);
int hhx_sort_graph_shape(const hhx_sort_graph *g, int32_t *shape, int64_t *ld, int64_t *n_edges);
int hhx_sort_graph_density(hhx_sort_graph *g, const double *len, int method, int64_t *n_flagged);
int hhx_sort_graph_fetch_flagged(hhx_sort_graph *g, int32_t *pairs);
int hhx_sort_graph_patch_len(hhx_sort_graph *g, int64_t n, const int32_t *pi, const int32_t *pj, const float *L);
int hhx_sort_graph_confidence(hhx_sort_graph *g, int32_t n_pairs, const int32_t *pair_a, const int32_t *pair_b, double *out);
int hhx_sort_graph_drop(hhx_sort_graph *g, int32_t a, int32_t b);
int hhx_sort_graph_aggregate(hhx_sort_graph *g, int32_t new_shape, const int32_t *map, int64_t *n_edges, int64_t *n_over);
int hhx_sort_graph_fetch_edges(hhx_sort_graph *g, int32_t *ei, int32_t *ej, float *w);
int hhx_sort_graph_fetch_over(hhx_sort_graph *g, int64_t *cells);
int hhx_sort_graph_patch_cells(hhx_sort_graph *g, int64_t n, const int64_t *cells, const int64_t *ordinal, const float *val);
int hhx_sort_graph_fetch_dense(hhx_sort_graph *g, int which, float *out);
int hhx_sort_graph_stats(const hhx_sort_graph *g, int64_t *values);
int hhx_sort_graph_destroy(hhx_sort_graph *g);
int hhx_sort_graph_confidence_device(hhx_sort_graph *g, int32_t n_pairs, const int32_t *pair_a, const int32_t *pair_b, double *maxs);
int hhx_sort_graph_fetch_confidence(hhx_sort_graph *g, double *out);
int hhx_sort_graph_forest(hhx_sort_graph *g, double cutoff, int64_t *n_chosen, int32_t *not_paths);
int hhx_sort_graph_fetch_forest(hhx_sort_graph *g, int32_t *eu, int32_t *ev, int32_t *label, int32_t *pos);
int hhx_sort_graph_forest_stats(const hhx_sort_graph *g, int64_t *values);

/* ---------------------------------------------------------------- `haphic sort`: fast sorting or ALLHiC (HapHiC_sort.py compare_fast_sort_and_allhic :645-724)
 * hhx_sort_verdict_sums — the sums behind the verdict, in place of the rotation loop :696-721 with its two find_lis passes :647-672 and its .index sweep
 *   :698-705 (csrc/hhx_sortverdict.hip).  value[n]: the compare_list :697-705 of rotation 0, element i of the fast-sort tour -> +(pos + 1) if its
 *   orientation equals the one in the ALLHiC tour, -(pos + 1) otherwise, pos its index there; the magnitudes are a permutation of 1 .. n.  len[n]: the
 *   contig lengths (order_len_dict), >= 0, summing to less than 2^62.  Rotation r is the sequence i = (r + k) mod n, k = 0 .. n - 1 (:720-721);
 *   sums[r - r0] = max(find_lis(forward), find_lis(reverse)) of rotation r for r0 <= r < r1 <= n - 1: the largest total length of a subsequence of one
 *   sign with strictly increasing signed values, 0 for an empty class — exact int64.  The n-th rotation is never looked at (:696).  The ratio rule
 *   :683-688, the 0.9 threshold :712-716, the early exit and the log lines stay with the caller, who asks for [0, 1) first and for the rest when that
 *   does not settle the verdict.  One wavefront per rotation; its Fenwick tree lives in LDS up to n = 4095 (lengths summing to less than 2^32: 4-byte
 *   cells) or 2047 (8-byte cells) by default, up to 40959 / 20479 with hhx_tune "sort_verdict_lds_n"; above that in a per-workgroup slab of a scratch
 *   buffer of at most 1 GiB in HBM, rotations taken in turns.  stats[HHX_SORT_VERDICT_N_STATS] (may be null): rotations run in the LDS form, in the HBM form, bytes per tree cell.
 *   Errors: n < 2, a value of 0 or of magnitude above n, a magnitude twice, a negative length, lengths summing to 2^62 or more, a rotation range
 *   outside [0, n - 1].  HHX_UNSUPPORTED: n above HHX_SORT_VERDICT_MAX_N (2^18 contigs; a rotation is n sequential steps). */
#define HHX_SORT_VERDICT_N_STATS 3
#define HHX_SORT_VERDICT_MAX_N 262144
int hhx_sort_verdict_sums(int32_t n, const int32_t *value, const int64_t *len, int32_t r0, int32_t r1, int64_t *sums, int64_t *stats);

/* ---------------------------------------------------------------- `haphic build`: FASTA reader and scaffold writer, haphic_amd/csrc/hhx_fasta.hip
 * hhx_fasta_open / hhx_fasta_open_bytes — parse_fasta, scripts/HapHiC_cluster.py:87-113, on a file or on bytes in host memory; the whole text goes
 *   to HBM in one piece.  Lines are Python's text-mode lines ('\n', "\r\n" and a lone '\r' end a line); a line that is empty after str.strip() is
 *   skipped :95; a line whose FIRST RAW byte is '>' is a header :97 and names the contig line.split()[0][1:] :98 ('>' alone and "> x" name ''); every
 *   other line is a sequence line: its bytes from the first to the last one that is no whitespace are kept, inner whitespace included, a-z folded to
 *   A-Z unless keep_letter_case :101-104.  Contigs stand in file order; a header without sequence lines is a contig of length 0.  The handle holds the
 *   sequences back to back in HBM, seq_off / seq_len per contig, and the names on the host.  Whitespace is the ASCII part of str.strip()'s.
 *   HHX_UNSUPPORTED (hhx_last_error() says why, no handle is made): a byte >= 0x80 (the reference decodes by the locale); a sequence line in front of
 *   the first header (the reference raises UnboundLocalError :102); text, sequences and one output slab beyond half of the device's memory; a path
 *   that is no regular file.  Contigs of one name are NOT detected here (fa_dict[ctg] = list() :99 overwrites): the caller compares the names.
 * hhx_fasta_counts: contigs, sequence bytes, name bytes (any pointer may be null).  hhx_fasta_table: seq_off [n_ctg], seq_len [n_ctg],
 *   name_off [n_ctg + 1] and the names one after the other (any pointer may be null).  hhx_fasta_sequences: the sequence bytes, copied to the host.
 * hhx_fasta_emit — the FASTA half of build_final_scaffolds, scripts/HapHiC_build.py:153-168: n_rec records in the order given; record r is
 *   ">name\n" (rec_names / rec_name_off [n_rec + 1]), then its sequence in lines of max_width bytes, each followed by '\n', the last one possibly
 *   shorter, none when the sequence is empty :159-160.  The sequence is the pieces [piece_off[r], piece_off[r + 1]) joined by Ns bytes of 'N' :84: piece k is
 *   contig piece_ctg[k], as it is or (piece_rev[k] != 0) reversed and mapped through ATCGNatcgn -> TAGCNtagcn :83, :127-129, every other byte
 *   unchanged; an unanchored contig :164-168 is a record of one forward piece.  All offsets are int64.  The file is produced in slabs of hhx_tune
 *   "fasta_slab" bytes on the device and written while the next slab is produced; *n_bytes (may be null) = its size.  It is complete and closed on return;
 *   after a failure it is removed.  HHX_UNSUPPORTED before the file is touched: max_width < 1, Ns < 0 or beyond 2^40, a record beyond 2^60 bytes. */
typedef struct hhx_fasta hhx_fasta;
int hhx_fasta_open(const char *path, int keep_letter_case, hhx_fasta **out);
int hhx_fasta_open_bytes(const uint8_t *text, int64_t n_bytes, int keep_letter_case, hhx_fasta **out);
int hhx_fasta_counts(const hhx_fasta *f, int64_t *n_ctg, int64_t *n_seq_bytes, int64_t *n_name_bytes);
int hhx_fasta_table(const hhx_fasta *f, int64_t *seq_off, int64_t *seq_len, int64_t *name_off, uint8_t *names);
int hhx_fasta_sequences(hhx_fasta *f, uint8_t *seq_host);
/* hhx_fasta_re_counts: hhx_count_re_sites (count_RE_sites :75-84) on the sequences the handle holds in HBM — the same matcher, no sequence byte crosses
 *   the bus.  Segments are in the handle's sequence coordinates (contig k: [seq_off[k], seq_off[k] + seq_len[k])) and checked against its sequence
 *   bytes; a match never crosses a segment end, so none straddles two contigs.
 * hhx_fasta_fetch: bytes [off, off + len) of the resident sequences into host memory; a range outside the sequences is refused (return 1). */
int hhx_fasta_re_counts(hhx_fasta *f, int64_t n_seg, const int64_t *seg_off, const int64_t *seg_len, int32_t n_sites, const uint8_t *sites,
                        const int32_t *site_len, int64_t *counts_host);
int hhx_fasta_fetch(hhx_fasta *f, int64_t off, int64_t len, uint8_t *out_host);
int hhx_fasta_emit(hhx_fasta *f, const char *path, int64_t n_rec, const uint8_t *rec_names, const int64_t *rec_name_off, const int64_t *piece_off,
                   const int32_t *piece_ctg, const uint8_t *piece_rev, int64_t Ns, int64_t max_width, int64_t *n_bytes);
/* hhx_fasta_emit_segments — the FASTA half of order_and_orient_groups, scripts/HapHiC_refsort.py:269-342, on an open handle: hhx_fasta_emit without a
 *   joiner, whose pieces are sub-ranges and N runs.  Piece k with piece_ctg[k] >= 0 is bytes [piece_start[k], piece_start[k] + piece_len[k]) of
 *   that contig (fa_dict[ctg][0][start - 1:end] :290, :305, :334), as they are or (piece_rev[k] != 0) reversed and mapped through ATCGNatcgn ->
 *   TAGCNtagcn, every other byte unchanged (revcom :155-160); piece_ctg[k] == -1 is piece_len[k] bytes of 'N' :293 (start and rev are not read).
 *   Header lines, lines of max_width bytes :319-320, no sequence line for an empty record, slabs of "fasta_slab" bytes each written while the next is
 *   produced, *n_bytes, the file complete and closed on return and removed after a failure: as hhx_fasta_emit.  HHX_UNSUPPORTED before the file is
 *   touched: a piece outside its contig, a negative length, max_width < 1, a record beyond 2^60 bytes.  Error: a contig id the table does not have. */
int hhx_fasta_emit_segments(hhx_fasta *f, const char *path, int64_t n_rec, const uint8_t *rec_names, const int64_t *rec_name_off, const int64_t *piece_off,
                            const int32_t *piece_ctg, const int64_t *piece_start, const int64_t *piece_len, const uint8_t *piece_rev, int64_t max_width,
                            int64_t *n_bytes);
int hhx_fasta_close(hhx_fasta *f);

/* ---------------------------------------------------------------- the GFA reader of parse_gfa, scripts/HapHiC_cluster.py:150-185 (haphic_amd/csrc/hhx_gfa.hip)
 * hhx_gfa_open / hhx_gfa_open_bytes: a file (through the pinned read-ahead of hhx_text_reader_open_raw) or bytes in host memory go to HBM in one piece and
 *   the table of the S records comes back; nothing stays on the device.  Lines are Python's text-mode lines ('\n', "\r\n" and a lone '\r' end a
 *   line).  A record is a line that begins with the two bytes 'S', TAB :160; field k is line.split('\t')[k] :161.  Per record, in file order: the
 *   bytes of field 1 :162, the integer behind the last ':' of field 3 (the whole field without one) :163, the same of field 4 :164.  An integer is
 *   served as 1 to 18 ASCII digits that end the field — or, where field 4 is the last field of the line, stand in front of the line break.
 *   HHX_UNSUPPORTED (hhx_last_error() names the line and the reason; no handle is made): a record with fewer than five fields (the TABs of the
 *   lines behind it are never credited to it); any other spelling of an integer (signs, blanks, underscores, more digits, none: Python's int()
 *   decides); a name longer than 255 bytes; a byte >= 0x80 anywhere in the text (the reference decodes the file by the locale); a text beyond half
 *   of the device's memory; a path that is no regular file.  No lane walks a line: a sequence field of any length costs a binary search in the
 *   scanned TAB counts of the 4 KB blocks.  The passes are grid-stride; the environment variable HHX_GFA_GRID (read at every launch) caps their
 *   workgroups, so that tests walk the loops on one and two of them.
 * hhx_gfa_counts: records, name bytes (any pointer may be null).  hhx_gfa_table: name_off [n_rec + 1], the names one after the other, len [n_rec],
 *   depth [n_rec] (any pointer may be null). */
typedef struct hhx_gfa hhx_gfa;
int hhx_gfa_open(const char *path, hhx_gfa **out);
int hhx_gfa_open_bytes(const uint8_t *text, int64_t n_bytes, hhx_gfa **out);
int hhx_gfa_counts(const hhx_gfa *g, int64_t *n_rec, int64_t *n_name_bytes);
int hhx_gfa_table(const hhx_gfa *g, int64_t *name_off, uint8_t *names, int64_t *len, int64_t *depth);
int hhx_gfa_close(hhx_gfa *g);

/* ---------------------------------------------------------------- `haphic refsort`: the PAF reader of parse_paf, scripts/HapHiC_refsort.py:81-134 (haphic_amd/csrc/hhx_paf.hip)
 * hhx_paf_open / hhx_paf_open_bytes: a file (through the pinned read-ahead of hhx_text_reader_open_raw) or bytes in host memory go to HBM in one piece and
 *   the table of its lines comes back; nothing stays on the device.  Lines are Python's text-mode lines ('\n', "\r\n" and a lone '\r' end a line); a
 *   line that is blank under line.strip() is skipped :88; field k is line.split()[k] :90 (runs of the ASCII whitespace of str.split(), leading
 *   whitespace ignored).  Per line, in file order: the ids of field 0 (the contig :93) and of field 5 (the reference sequence :93) in ONE name table
 *   whose names stand in first-seen order (field 0 of a line before its field 5), the integers of fields 2, 3 :93, 7, 8 :107 and 11 :91, and
 *   whether field 4 is exactly "+" :94.  An integer is served as 1 to 18 ASCII digits that are the whole field.
 *   HHX_UNSUPPORTED (hhx_last_error() names the line and the reason; no handle is made): a line that is not blank with fewer than 12 fields (the
 *   reference raises IndexError); any other spelling of an integer (signs, underscores, more digits: Python's int() decides) — of EVERY line, also
 *   where the reference would not convert the field (:91 mapq 0, :101-105 contigs it skips): handing such a file back whole is still exact; a name
 *   longer than 255 bytes; a byte >= 0x80 anywhere in the text; a text beyond half of the device's memory, or whose per-line tables (288 bytes a line) do not fit beside
 *   it there; 2^30 lines or more; a path that is no
 *   regular file.  No lane walks a line: only the first 12 fields are located, each by a binary search in the scanned field-start counts of the
 *   4 KB blocks, so a cg:Z: tag of any length costs nothing.  The passes are grid-stride; the environment variable HHX_PAF_GRID (read at every
 *   launch) caps their workgroups, so that tests walk the loops on one and two of them.
 * hhx_paf_counts: lines, names, name bytes (any pointer may be null).  hhx_paf_table: name_off [n_names + 1], the names one after the other, query
 *   and target [n_rec] (name ids), query_start, query_end, target_start, target_end, mapq [n_rec], plus [n_rec] (any pointer may be null). */
typedef struct hhx_paf hhx_paf;
int hhx_paf_open(const char *path, hhx_paf **out);
int hhx_paf_open_bytes(const uint8_t *text, int64_t n_bytes, hhx_paf **out);
int hhx_paf_counts(const hhx_paf *g, int64_t *n_rec, int64_t *n_names, int64_t *n_name_bytes);
int hhx_paf_table(const hhx_paf *g, int64_t *name_off, uint8_t *names, int32_t *query, int32_t *target, int64_t *query_start, int64_t *query_end,
                  int64_t *target_start, int64_t *target_end, int64_t *mapq, uint8_t *plus);
int hhx_paf_close(hhx_paf *g);

/* hhx_lis_sums — both find_lis sums (scripts/HapHiC_refsort.py:175-214, called twice per group :246-247) of n_seq sequences in one call
 *   (csrc/hhx_sortverdict.hip, the wave step of hhx_sort_verdict_sums).  Sequence s is elements ptr[s] .. ptr[s + 1] (ptr[0] = 0); value[]: a signed
 *   64-bit key (the caller passes 2 * order: orders are multiples of 0.5), len[]: the weight.  The forward class is the elements with value >= 0
 *   :182-183, the reverse class those with value <= 0 :184-185; within a class an element whose value stood earlier in the sequence is dropped
 *   :186-187; sums_f[s] / sums_r[s] = the largest total weight of a subsequence of the class with strictly increasing values :199-207, 0 for an empty
 *   class :192-193 — exact int64.  The ranks and the dropping of repeats are computed by the entry's host code; one wavefront per (sequence, class);
 *   the tree in LDS up to hhx_tune "sort_verdict_lds_n" kept elements and in HBM scratch above, 4-byte cells while every sequence's weights sum to
 *   less than 2^32 and 8-byte cells otherwise.  HHX_UNSUPPORTED: a weight <= 0, the weights of one sequence summing to 2^62 or more, a sequence
 *   beyond HHX_SORT_VERDICT_MAX_N elements. */
int hhx_lis_sums(int64_t n_seq, const int64_t *ptr, const int64_t *value, const int64_t *len, int64_t *sums_f, int64_t *sums_r);

#ifdef __cplusplus
}
#endif
#endif /* HAPHIC_HIP_H */
