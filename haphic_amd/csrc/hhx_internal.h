// What the .hip files of libhaphic_hip.so call in each other beside the C ABI of include/haphic_hip.h: declared here once and included by
// the file that defines a function as well as by the files that call it, so that the compiler checks every definition against its uses.
#pragma once
#include "hhx_common.h"

struct hhx_ingest;      // hhx_ingest.h

// ---- hhx_runtime.hip
int hhx_csr_alloc_internal(i32 n_rows, i32 n_cols, i64 nnz, hhx_csr **out);

// ---- hhx_expand.hip
// b is the L1-normalised link matrix described by lk (hhx_common.h): the fused iteration with the window class streaming b by link count
int hhx_expand_class_stream(const hhx_csr *a, const hhx_csr *b, const hhx_links_operand *lk, int fx_shift, double inflation, double pruning, hhx_csr **out,
                            i64 *n_products, i64 *nnz_expanded);
// the rows of a * b as a plain float32 block (the inflation sweep); 2: the block itself does not fit
int hhx_expand_dense_impl(const hhx_csr *a, const hhx_csr *b, const hhx_links_operand *lk, int fx_shift, hhx_dense **out, i64 *n_products, i64 *nnz_expanded);
// C = A * B through the fused kernels in plain-product mode (hhx_spgemm's fast path)
int hhx_expand_raw(const hhx_csr *a, const hhx_csr *b, int fx_shift, hhx_csr **out, i64 *n_products);
// the pools of the next fused iteration on this thread sized from the one before (mcl()'s loop)
void hhx_expand_set_hint(i64 out, i64 cand);
void hhx_expand_last_demand(i64 *out, i64 *cand);
// how the dense block of all rows is stored — 1: the square, 2: the upper block triangle, 0: neither fits
int hhx_dense_layout(i32 n_rows, i32 n_cols, i64 nnz_b);

// ---- hhx_resites.hip
// hhx_count_re_sites on sequence bytes that lie in device memory already (seq_len of them and one readable byte behind): segments and sites from the
// host, counts back to it; `who` names the entry in the error text
int hhx_count_re_sites_device(const char *who, const unsigned char *seq, i64 seq_len, i64 n_seg, const i64 *seg_off, const i64 *seg_len, i32 n_sites,
                              const uint8_t *sites, const i32 *site_len, i64 *counts_host);

// ---- hhx_reassign.hip
// hhx_reassign_create with the three key arrays in device memory (copied device to device)
int hhx_reassign_create_device(const char *who, i64 n_keys, const i32 *frag_i, const i32 *frag_j, const i64 *links, i32 n_ctg, const i32 *group_host,
                               i32 n_groups, hhx_reassign **out);

// ---- hhx_ingest.hip
// the dict-ordered tables (made on first use)
int hhx_ingest_ordered_full_device(hhx_ingest *h, const i32 **fi, const i32 **fj);
