"""ctypes binding of libhaphic_hip.so (include/haphic_hip.h).

This is the stub a HapHiC maintainer would add next to scripts/HapHiC_cluster.py.
There is NO CPU fallback: if the HIP library is missing or no GPU is visible, loading / the first
call raises, exactly as a missing sparse_dot_mkl would — but loudly.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get('HAPHIC_HIP_SO') or os.path.join(_HERE, 'libhaphic_hip.so')      # (the override: the sanitizer build of build.build_asan)

c_i32p = C.POINTER(C.c_int32)
c_i64p = C.POINTER(C.c_int64)
c_f32p = C.POINTER(C.c_float)
c_f64p = C.POINTER(C.c_double)
c_u8p = C.POINTER(C.c_uint8)
c_vpp = C.POINTER(C.c_void_p)


class IngestConfig(C.Structure):
    _fields_ = [('n_ctg', C.c_int32), ('n_frag', C.c_int32),
                ('ctg_rank', c_i32p), ('ctg_len', c_i64p), ('ctg_frag0', c_i32p), ('ctg_split', c_u8p),
                ('frag_rank', c_i32p), ('frag_len', c_i64p), ('frag_nx', c_u8p),
                ('bin_size', C.c_int64), ('flank', C.c_int64), ('bins', C.c_int32), ('skip_intra', C.c_int32),
                ('expected_keys', C.c_int64)]


# name -> (restype, argtypes); every symbol include/haphic_hip.h declares
SIGNATURES = {
    'hhx_last_error': (C.c_char_p, []),
    'hhx_version': (C.c_int, []),
    'hhx_device_count': (C.c_int, [C.POINTER(C.c_int)]),
    'hhx_set_device': (C.c_int, [C.c_int]),
    'hhx_set_stream': (C.c_int, [C.c_void_p]),
    'hhx_synchronize': (C.c_int, []),
    'hhx_pool_trim': (C.c_int, []),
    'hhx_pool_trim_keep': (C.c_int, [C.c_int64]),
    'hhx_pool_prewarm': (C.c_int, [C.c_int32, c_i64p]),
    'hhx_tune': (C.c_int, [C.c_char_p, C.c_int64]),
    'hhx_profile_enable': (C.c_int, [C.c_int]),
    'hhx_profile_reset': (C.c_int, []),
    'hhx_profile_get': (C.c_int, [C.c_char_p, c_f64p, c_i64p]),
    'hhx_profile_counter': (C.c_int, [C.c_char_p, c_i64p]),
    'hhx_csr_from_host': (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, c_vpp]),
    'hhx_csr_from_device': (C.c_int, [C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, c_vpp]),
    'hhx_csr_shape': (C.c_int, [C.c_void_p, c_i32p, c_i32p, c_i64p]),
    'hhx_csr_to_host': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'hhx_csr_device_ptrs': (C.c_int, [C.c_void_p, c_vpp, c_vpp, c_vpp]),
    'hhx_csr_copy': (C.c_int, [C.c_void_p, c_vpp]),
    'hhx_csr_row_block': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, c_vpp]),
    'hhx_csr_free': (C.c_int, [C.c_void_p]),
    'hhx_normalize_l1': (C.c_int, [C.c_void_p]),
    'hhx_inflate': (C.c_int, [C.c_void_p, C.c_double]),
    'hhx_prune': (C.c_int, [C.c_void_p, C.c_double, c_vpp]),
    'hhx_inflate_prune': (C.c_int, [C.c_void_p, C.c_double, C.c_double, c_vpp]),
    'hhx_spgemm': (C.c_int, [C.c_void_p, C.c_void_p, c_vpp]),
    'hhx_spgemm_ex': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, c_vpp, c_i64p]),
    'hhx_expand_inflate_prune': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, c_vpp, c_i64p, c_i64p]),
    'hhx_link_weights': (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int32, C.c_void_p, C.c_void_p,
                                   C.c_double, c_i64p]),
    'hhx_group_link_sums': (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    'hhx_row_products': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'hhx_expand_links': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int, C.c_double, C.c_double, c_vpp, c_i64p, c_i64p]),
    'hhx_convergence_stat': (C.c_int, [C.c_void_p, C.c_void_p, c_f32p]),
    'hhx_mcl': (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_double, c_vpp, C.POINTER(C.c_int),
                          C.POINTER(C.c_int), C.c_void_p]),
    'hhx_mcl_normalized': (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_double, c_vpp, C.POINTER(C.c_int),
                                     C.POINTER(C.c_int), C.c_void_p]),
    'hhx_mcl_links': (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_double, c_vpp, C.POINTER(C.c_int),
                                C.POINTER(C.c_int), C.c_void_p]),
    'hhx_interpret': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, c_i32p]),
    'hhx_dict_to_matrix': (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int32, C.c_void_p,
                                     C.c_int32, C.c_int, C.c_void_p, c_i32p, c_vpp]),
    'hhx_count_re_sites': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    'hhx_rank_sums': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    'hhx_ingest_create': (C.c_int, [C.POINTER(IngestConfig), c_vpp]),
    'hhx_ingest_push': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    'hhx_ingest_push64': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    'hhx_ingest_finalize': (C.c_int, [C.c_void_p, c_i64p, c_i64p]),
    'hhx_ingest_fetch': (C.c_int, [C.c_void_p] + [C.c_void_p] * 8),
    'hhx_ingest_flank_device': (C.c_int, [C.c_void_p, c_vpp, c_vpp, c_vpp]),
    'hhx_ingest_flank_count_device': (C.c_int, [C.c_void_p, c_vpp]),
    'hhx_ingest_destroy': (C.c_int, [C.c_void_p]),
    'hhx_ingest_keep_pairs': (C.c_int, [C.c_void_p, C.c_int]),
    'hhx_csr_vstack': (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), c_vpp]),
    'hhx_mem_info': (C.c_int, [c_i64p, c_i64p]),
    'hhx_pool_cached_bytes': (C.c_int, [c_i64p]),
    'hhx_csr_pack_block': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    'hhx_csr_unpack_blocks': (C.c_int, [C.c_int32, c_i64p, c_i64p, C.c_void_p, C.c_int64, C.c_int32, c_vpp]),
    'hhx_inflate_prune_keep': (C.c_int, [C.c_void_p, C.c_double, C.c_double, c_vpp]),
    'hhx_mcl_resume': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_double, c_vpp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p]),
    'hhx_expand_links_dense': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int, C.c_int, c_vpp, c_i64p, c_i64p]),
    'hhx_links_integer_ok': (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'hhx_links_plan': (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'hhx_dense_device': (C.c_int, [C.c_void_p, c_vpp, c_i64p, c_i32p, c_i32p]),
    'hhx_dense_inflate_prune': (C.c_int, [C.c_void_p, C.c_double, C.c_double, c_vpp]),
    'hhx_copy_rect_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64]),
    'hhx_transpose_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64]),
    'hhx_dense_inflate_prune_multi': (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.c_double, c_vpp]),
    'hhx_dense_shape': (C.c_int, [C.c_void_p, c_i32p, c_i32p, c_i64p]),
    'hhx_dense_free': (C.c_int, [C.c_void_p]),
    'hhx_shard_create': (C.c_int, [C.c_void_p, C.c_void_p, c_vpp]),
    'hhx_shard_first': (C.c_int, [C.c_void_p, c_vpp]),
    'hhx_rank_first': (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, c_i32p]),
    'hhx_shard_emit': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, c_i32p, c_vpp, c_vpp, c_i64p]),
    'hhx_rows_from_entries': (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int, c_vpp]),
    'hhx_rows_from_runs': (C.c_int, [C.c_int32, c_i64p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int, c_vpp]),
    'hhx_shard_destroy': (C.c_int, [C.c_void_p]),
    'hhx_pairs_parser_create': (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    'hhx_pairs_parse': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, c_i64p, c_i64p]),
    'hhx_pairs_parser_arrays': (C.c_int, [C.c_void_p] + [C.POINTER(C.c_void_p)] * 5),
    'hhx_pairs_parser_fetch': (C.c_int, [C.c_void_p] + [C.c_void_p] * 5),
    'hhx_pairs_parser_set_wide': (C.c_int, [C.c_void_p, C.c_int]),
    'hhx_pairs_parser_fetch64': (C.c_int, [C.c_void_p] + [C.c_void_p] * 5),
    'hhx_pairs_parser_bed_host': (C.c_int, [C.c_void_p, c_vpp, c_i64p]),
    'hhx_pairs_parser_destroy': (C.c_int, [C.c_void_p]),
    'hhx_pairs_format': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, c_i64p]),
    'hhx_bam_open': (C.c_int, [C.c_char_p, C.c_int, c_vpp]),
    'hhx_bam_header': (C.c_int, [C.c_void_p, c_i32p, C.POINTER(C.c_char_p), c_i64p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    'hhx_bam_next': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int32, C.c_void_p, C.c_int64, c_i64p, c_vpp, c_vpp, c_vpp, c_vpp]),
    'hhx_bam_fetch': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'hhx_bam_close': (C.c_int, [C.c_void_p]),
    'hhx_contact_map_create': (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                         C.c_int32, c_vpp]),
    'hhx_contact_map_push': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int32, c_i64p]),
    'hhx_contact_map_fetch': (C.c_int, [C.c_void_p, C.c_void_p]),
    'hhx_contact_map_device': (C.c_int, [C.c_void_p, c_vpp, c_i32p]),
    'hhx_contact_map_destroy': (C.c_int, [C.c_void_p]),
    'hhx_plotnorm_create': (C.c_int, [C.c_void_p, C.c_int32, c_vpp, c_i64p, c_i64p, c_i32p]),
    'hhx_plotnorm_set_blocks': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    'hhx_plotnorm_balance': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'hhx_plotnorm_fetch_x': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'hhx_plotnorm_apply': (C.c_int, [C.c_void_p, C.c_void_p]),
    'hhx_plotnorm_median': (C.c_int, [C.c_void_p, C.c_int32, c_i64p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    'hhx_plotnorm_matvec': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    'hhx_plotnorm_destroy': (C.c_int, [C.c_void_p]),
    'hhx_select_middle_u64': (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    'hhx_ingest_fetch_ht_order': (C.c_int, [C.c_void_p, C.c_void_p]),
    'hhx_ingest_keep_frag_pairs': (C.c_int, [C.c_void_p, C.c_int]),
    'hhx_ingest_fetch_frag_pairs': (C.c_int, [C.c_void_p, c_i64p, C.c_void_p, C.c_void_p]),
    'hhx_ingest_fetch_pairs': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'hhx_ingest_set_ordinal_base': (C.c_int, [C.c_void_p, C.c_int64]),
    'hhx_ingest_concordance': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    'hhx_ingest_drop_links': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, c_i64p, c_i64p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'hhx_allelic_nonmax': (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     c_i32p]),
    'hhx_lsap_small': (C.c_int, [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    'hhx_ingest_group_stats': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    'hhx_reassign_create': (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, c_vpp]),
    'hhx_reassign_cells': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'hhx_reassign_round': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double,
                                     C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int64)]),
    'hhx_reassign_pair_sums': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    'hhx_reassign_destroy': (C.c_int, [C.c_void_p]),
    'hhx_reassign_create_from_pickle': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int), c_vpp]),
    'hhx_group_stats': (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'hhx_ingest_link_matrix': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.c_void_p, c_i32p, c_vpp]),
    'hhx_ingest_table_device': (C.c_int, [C.c_void_p, C.c_int, c_i64p, c_vpp, c_vpp, c_vpp, c_vpp, c_vpp]),
    'hhx_ingest_push_table': (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'hhx_ingest_fetch_flank_values': (C.c_int, [C.c_void_p, C.c_void_p]),
    'hhx_ingest_fetch_ht_items': (C.c_int, [C.c_void_p, c_i64p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'hhx_ingest_write_clm': (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, c_i64p, c_i64p]),
    'hhx_write_link_pickle': (C.c_int, [C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, c_i64p]),
    'hhx_ingest_write_clm_async': (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_int]),
    'hhx_ingest_write_link_pickle_async': (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_int32, C.c_void_p, C.c_void_p]),
    'hhx_write_link_pickle_async': (C.c_int, [C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    'hhx_byte_sink_open': (C.c_int, [C.c_char_p, C.c_int64, C.c_int64, c_vpp]),
    'hhx_byte_sink_reserve': (C.c_int, [C.c_void_p, C.c_int64, c_vpp]),
    'hhx_byte_sink_commit': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    'hhx_byte_sink_close': (C.c_int, [C.c_void_p, c_i64p]),
    'hhx_byte_sink_open_deferred': (C.c_int, [C.c_char_p, C.c_int64, C.c_int64, c_vpp]),
    'hhx_byte_sink_set_base': (C.c_int, [C.c_void_p, C.c_int64]),
    'hhx_pairs_parser_set_bed_sink': (C.c_int, [C.c_void_p, C.c_void_p]),
    'hhx_text_reader_open': (C.c_int, [C.c_char_p, C.c_int64, C.c_int, c_vpp]),
    'hhx_text_reader_open_bgzf': (C.c_int, [C.c_char_p, C.c_int64, C.c_int, c_vpp]),
    'hhx_text_reader_open_range': (C.c_int, [C.c_char_p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, c_vpp]),
    'hhx_text_reader_open_raw': (C.c_int, [C.c_char_p, C.c_int64, C.c_int, c_vpp]),
    'hhx_text_reader_next': (C.c_int, [C.c_void_p, c_vpp, c_i64p]),
    'hhx_text_reader_close': (C.c_int, [C.c_void_p]),
    'hhx_clm_split_create': (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, c_vpp]),
    'hhx_clm_split_push': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int]),
    'hhx_clm_split_file': (C.c_int, [C.c_void_p, C.c_char_p, C.c_int64, C.c_int]),
    'hhx_clm_split_finish': (C.c_int, [C.c_void_p, c_i64p, c_i64p, C.c_void_p]),
    'hhx_clm_split_stats': (C.c_int, [C.c_void_p, C.c_void_p]),
    'hhx_clm_split_destroy': (C.c_int, [C.c_void_p]),
    'hhx_pickle_open': (C.c_int, [C.c_char_p, c_vpp]),
    'hhx_pickle_sizes': (C.c_int, [C.c_void_p, c_i64p, c_i32p, c_i64p, C.POINTER(C.c_int)]),
    'hhx_pickle_fetch': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'hhx_pickle_free': (C.c_int, [C.c_void_p]),
    'hhx_pickle_group_heads': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, c_i64p]),
    'hhx_pickle_group_heads_fetch': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'hhx_files_pending': (C.c_int, [c_i64p, c_i64p]),
    'hhx_files_join': (C.c_int, [c_i64p]),
    'hhx_correct_create': (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, c_vpp]),
    'hhx_correct_push': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    'hhx_correct_finalize': (C.c_int, [C.c_void_p, c_i64p]),
    'hhx_correct_export': (C.c_int, [C.c_void_p, c_i32p, c_i64p, c_i64p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int]),
    'hhx_correct_absorb': (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int]),
    'hhx_correct_shape': (C.c_int, [C.c_void_p, c_i32p, c_i64p, c_i64p]),
    'hhx_correct_fetch_segments': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'hhx_correct_fetch_coverage': (C.c_int, [C.c_void_p, C.c_void_p]),
    'hhx_correct_fetch_pairs': (C.c_int, [C.c_void_p, C.c_void_p]),
    'hhx_correct_detect': (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_int64, C.c_void_p, C.c_void_p, c_i64p]),
    'hhx_correct_fetch_break_points': (C.c_int, [C.c_void_p, C.c_void_p]),
    'hhx_correct_break': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'hhx_correct_destroy': (C.c_int, [C.c_void_p]),
    'hhx_remap_create': (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, c_vpp]),
    'hhx_remap_apply': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    'hhx_remap_destroy': (C.c_int, [C.c_void_p]),
    'hhx_sort_graph_create': (C.c_int, [C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, c_vpp]),
    'hhx_sort_graph_shape': (C.c_int, [C.c_void_p, c_i32p, c_i64p, c_i64p]),
    'hhx_sort_graph_density': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, c_i64p]),
    'hhx_sort_graph_fetch_flagged': (C.c_int, [C.c_void_p, C.c_void_p]),
    'hhx_sort_graph_patch_len': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    'hhx_sort_graph_confidence': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    'hhx_sort_graph_drop': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    'hhx_sort_graph_aggregate': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, c_i64p, c_i64p]),
    'hhx_sort_graph_fetch_edges': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'hhx_sort_graph_fetch_over': (C.c_int, [C.c_void_p, C.c_void_p]),
    'hhx_sort_graph_patch_cells': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    'hhx_sort_graph_fetch_dense': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    'hhx_sort_graph_stats': (C.c_int, [C.c_void_p, C.c_void_p]),
    'hhx_sort_graph_destroy': (C.c_int, [C.c_void_p]),
    'hhx_sort_graph_confidence_device': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    'hhx_sort_graph_fetch_confidence': (C.c_int, [C.c_void_p, C.c_void_p]),
    'hhx_sort_graph_forest': (C.c_int, [C.c_void_p, C.c_double, c_i64p, c_i32p]),
    'hhx_sort_graph_fetch_forest': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'hhx_sort_graph_forest_stats': (C.c_int, [C.c_void_p, C.c_void_p]),
    'hhx_sort_verdict_sums': (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    'hhx_fasta_open': (C.c_int, [C.c_char_p, C.c_int, c_vpp]),
    'hhx_fasta_open_bytes': (C.c_int, [C.c_void_p, C.c_int64, C.c_int, c_vpp]),
    'hhx_fasta_counts': (C.c_int, [C.c_void_p, c_i64p, c_i64p, c_i64p]),
    'hhx_fasta_table': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'hhx_fasta_sequences': (C.c_int, [C.c_void_p, C.c_void_p]),
    'hhx_fasta_emit': (C.c_int, [C.c_void_p, C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                 c_i64p]),
    'hhx_fasta_re_counts': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    'hhx_fasta_fetch': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    'hhx_fasta_close': (C.c_int, [C.c_void_p]),
    'hhx_gfa_open': (C.c_int, [C.c_char_p, c_vpp]),
    'hhx_gfa_open_bytes': (C.c_int, [C.c_void_p, C.c_int64, c_vpp]),
    'hhx_gfa_counts': (C.c_int, [C.c_void_p, c_i64p, c_i64p]),
    'hhx_gfa_table': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'hhx_gfa_close': (C.c_int, [C.c_void_p]),
    'hhx_fasta_emit_segments': (C.c_int, [C.c_void_p, C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_int64, c_i64p]),
    'hhx_paf_open': (C.c_int, [C.c_char_p, c_vpp]),
    'hhx_paf_open_bytes': (C.c_int, [C.c_void_p, C.c_int64, c_vpp]),
    'hhx_paf_counts': (C.c_int, [C.c_void_p, c_i64p, c_i64p, c_i64p]),
    'hhx_paf_table': (C.c_int, [C.c_void_p] + [C.c_void_p] * 10),
    'hhx_paf_close': (C.c_int, [C.c_void_p]),
    'hhx_lis_sums': (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'hhx_dmat_from_host': (C.c_int, [C.c_int32, C.c_void_p, c_vpp]),
    'hhx_dmat_from_csr': (C.c_int, [C.c_void_p, c_vpp]),
    'hhx_dmat_to_host': (C.c_int, [C.c_void_p, C.c_void_p]),
    'hhx_dmat_to_csr': (C.c_int, [C.c_void_p, c_vpp]),
    'hhx_dmat_copy': (C.c_int, [C.c_void_p, c_vpp]),
    'hhx_dmat_shape': (C.c_int, [C.c_void_p, c_i32p, c_i64p, c_i64p]),
    'hhx_dmat_free': (C.c_int, [C.c_void_p]),
    'hhx_dmat_gemm': (C.c_int, [C.c_void_p, C.c_void_p, c_vpp]),
    'hhx_dmat_normalize_l1': (C.c_int, [C.c_void_p]),
    'hhx_dmat_prune': (C.c_int, [C.c_void_p, C.c_double, c_vpp]),
    'hhx_dmat_power': (C.c_int, [C.c_void_p, C.c_int, c_vpp]),
    'hhx_dmat_mcl': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_double, c_vpp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
}

_lib = None


def load():
    """dlopen the library and bind every declared symbol (does not touch the GPU)."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise ImportError('haphic_amd: %s is missing — build it with `python -m haphic_amd.build` '
                              '(hipcc --offload-arch=gfx950); there is no CPU fallback' % SO_PATH)
        # torch ships its own libamdhip64.so.7 / libhsa-runtime64.so.1 and dlopens them by path; two HIP
        # runtimes in one process cannot both own the GPU.  Importing torch first makes the dynamic
        # linker resolve this library's DT_NEEDED libamdhip64.so.7 to the copy torch already loaded,
        # so torch tensors (device memory, streams, RCCL) and these kernels share one runtime.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = C.CDLL(SO_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)      # AttributeError if the .so does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


HHX_UNSUPPORTED = 2                  # "not served here": the caller takes the reference's path, the handle is untouched


def last_error():
    return load().hhx_last_error().decode('utf-8', 'replace')


def check(rc):
    if rc != 0:
        raise RuntimeError('libhaphic_hip: ' + last_error())


def check_served(rc, unsupported=None):
    """check(rc), except for HHX_UNSUPPORTED: raises unsupported(last_error()), or with no class given returns False (else True)"""
    if rc == HHX_UNSUPPORTED:
        if unsupported is None:
            return False
        raise unsupported(last_error())
    check(rc)
    return True


_PY_ERRORS = {'IndexError': IndexError, 'ValueError': ValueError}


def check_py(rc):
    """check(rc) for the calls that fail as the reference's own statement would: a message 'IndexError: ...' / 'ValueError: ...' raises that
    exception with the text behind the prefix"""
    if rc:
        msg = last_error()
        kind, sep, text = msg.partition(': ')
        if sep and kind in _PY_ERRORS:
            raise _PY_ERRORS[kind](text)
        raise RuntimeError('libhaphic_hip: ' + msg)


def new_handle(symbol, *args):
    """symbol(*args, &out) of the library -> the handle it left in that last parameter"""
    out = C.c_void_p()
    check(getattr(load(), symbol)(*args, C.byref(out)))
    return out


class Handle:
    """One handle of the library: self.h, released once by the symbol the subclass names in _release — by close() (free() and destroy() are the
    same call under the names older callers use), at the end of a `with` block, or by the finaliser when nobody did."""
    _release = None
    _finalise = True

    def __init__(self, handle):
        self.h = handle if isinstance(handle, C.c_void_p) else C.c_void_p(handle)

    def close(self):
        h, self.h = getattr(self, 'h', None), None
        if h:                           # neither None nor a null pointer
            getattr(load(), self._release)(h)

    def free(self):
        return self.close()

    def destroy(self):
        return self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            if self._finalise:
                self.close()
        except Exception:
            pass


def device_count():
    n = C.c_int(0)
    check(load().hhx_device_count(C.byref(n)))
    return n.value


def set_device(i):
    check(load().hhx_set_device(int(i)))


def synchronize():
    check(load().hhx_synchronize())


def pool_trim(keep_bytes=None):
    """the pool's cached blocks back to the driver; keep_bytes: all but that much of them (hhx_pool_trim_keep)"""
    check(load().hhx_pool_trim() if keep_bytes is None else load().hhx_pool_trim_keep(int(keep_bytes)))


def tune(name, value):
    """which kernel class / arithmetic / layout the calls take (hhx_tune; same results under every setting); None: back to the default"""
    check(load().hhx_tune(name.encode(), -2 ** 63 if value is None else int(value)))


def profile_enable(on=True):
    check(load().hhx_profile_enable(int(on)))


def profile_reset():
    check(load().hhx_profile_reset())


def profile_get(kernel):
    ms, n = C.c_double(0), C.c_int64(0)
    check(load().hhx_profile_get(kernel.encode(), C.byref(ms), C.byref(n)))
    return ms.value, n.value


def profile_counter(name):
    v = C.c_int64(0)
    check(load().hhx_profile_counter(name.encode(), C.byref(v)))
    return v.value


def ptr(a):
    """host pointer of a C-contiguous numpy array (or None)"""
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class DeviceCSR(Handle):
    """Device-resident CSR(T) == the reference's CSC(M) triple (hhx_csr handle)."""
    _release = 'hhx_csr_free'

    @classmethod
    def from_arrays(cls, indptr, indices, data, n_cols=None):
        indptr, indices = np.asarray(indptr), np.asarray(indices)
        if len(indptr) and int(indptr[-1]) > np.iinfo(np.int32).max:       # a scipy matrix with int64 indices: do not wrap
            raise ValueError('matrix with {} entries exceeds the int32 index range of hhx_csr'.format(int(indptr[-1])))
        if indices.size and (int(indices.max()) > np.iinfo(np.int32).max or int(indices.min()) < 0):
            raise ValueError('column index outside the int32 range')
        indptr = np.ascontiguousarray(indptr, np.int32)
        indices = np.ascontiguousarray(indices, np.int32)
        data = np.ascontiguousarray(data, np.float32)
        n_rows = len(indptr) - 1
        return cls(new_handle('hhx_csr_from_host', n_rows, n_rows if n_cols is None else n_cols, ptr(indptr), ptr(indices), ptr(data)))

    @classmethod
    def from_scipy_csc(cls, m):
        """scipy CSC of M, canonicalised (sorted indices, duplicates summed) like the reference's own
        intermediate matrices after `.power()` (scipy _deduped_data)."""
        m = m.tocsc()
        if not m.has_canonical_format:
            m = m.copy()
            m.sum_duplicates()
        return cls.from_arrays(m.indptr, m.indices, m.data.astype(np.float32, copy=False), n_cols=m.shape[0])

    @classmethod
    def from_device(cls, n_rows, n_cols, nnz, indptr_ptr, indices_ptr, data_ptr):
        return cls(new_handle('hhx_csr_from_device', n_rows, n_cols, nnz, C.c_void_p(indptr_ptr), C.c_void_p(indices_ptr), C.c_void_p(data_ptr)))

    @property
    def shape3(self):
        r, c, z = C.c_int32(), C.c_int32(), C.c_int64()
        check(load().hhx_csr_shape(self.h, C.byref(r), C.byref(c), C.byref(z)))
        return r.value, c.value, z.value

    @property
    def nnz(self):
        return self.shape3[2]

    def to_arrays(self):
        r, c, z = self.shape3
        indptr = np.empty(r + 1, np.int32)
        indices = np.empty(z, np.int32)
        data = np.empty(z, np.float32)
        check(load().hhx_csr_to_host(self.h, ptr(indptr), ptr(indices), ptr(data)))
        return indptr, indices, data

    def to_scipy_csc(self):
        import scipy.sparse as sp
        r, c, _ = self.shape3
        indptr, indices, data = self.to_arrays()
        return sp.csc_matrix((data, indices, indptr), shape=(c, r))

    def device_ptrs(self):
        a, b, d = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(load().hhx_csr_device_ptrs(self.h, C.byref(a), C.byref(b), C.byref(d)))
        return a.value or 0, b.value or 0, d.value or 0

    def copy(self):
        return DeviceCSR(new_handle('hhx_csr_copy', self.h))

    def row_block(self, r0, r1):
        return DeviceCSR(new_handle('hhx_csr_row_block', self.h, r0, r1))


class DenseMatrix(Handle):
    """Device-resident n x n float32 matrix M of the --dense_matrix mode (hhx_dmat handle; stored transposed and padded, every array in and
    out is M as the reference has it)."""
    _release = 'hhx_dmat_free'

    @classmethod
    def from_numpy(cls, m):
        m = np.ascontiguousarray(m, np.float32)
        if m.ndim != 2 or m.shape[0] != m.shape[1]:
            raise ValueError('the dense mode needs a square matrix, got shape {}'.format(m.shape))
        return cls(new_handle('hhx_dmat_from_host', m.shape[0], ptr(m)))

    @classmethod
    def from_csr(cls, t):
        """t: DeviceCSR, CSR(T) == CSC(M); densified on the device"""
        return cls(new_handle('hhx_dmat_from_csr', t.h))

    @property
    def shape(self):
        n = C.c_int32()
        check(load().hhx_dmat_shape(self.h, C.byref(n), None, None))
        return n.value, n.value

    @property
    def nbytes(self):
        b = C.c_int64()
        check(load().hhx_dmat_shape(self.h, None, None, C.byref(b)))
        return b.value

    def to_numpy(self):
        n = self.shape[0]
        out = np.empty((n, n), np.float32)
        check(load().hhx_dmat_to_host(self.h, ptr(out)))
        return out

    def to_csr(self):
        return DeviceCSR(new_handle('hhx_dmat_to_csr', self.h))

    def copy(self):
        return DenseMatrix(new_handle('hhx_dmat_copy', self.h))


def dmat_gemm(a, b):
    """a @ b of two DenseMatrix (float32 in, float32 accumulate, k ascending)"""
    return DenseMatrix(new_handle('hhx_dmat_gemm', a.h, b.h))


def dmat_normalize_l1(m):
    check(load().hhx_dmat_normalize_l1(m.h))
    return m


def dmat_prune(m, pruning):
    return DenseMatrix(new_handle('hhx_dmat_prune', m.h, float(pruning)))


def dmat_power(m, expansion):
    return DenseMatrix(new_handle('hhx_dmat_power', m.h, int(expansion)))


def dmat_mcl(pre_expanded, expansion, inflation, max_iter, pruning, done=0):
    """mcl(..., dense_matrix=True) :2026-2062 -> (DenseMatrix, rounds, converged); done = k, max_iter = k + 1: exactly round k"""
    out, n_iter, conv = C.c_void_p(), C.c_int(0), C.c_int(0)
    check(load().hhx_dmat_mcl(pre_expanded.h, int(done), int(expansion), float(inflation), int(max_iter), float(pruning), C.byref(out),
                              C.byref(n_iter), C.byref(conv)))
    return DenseMatrix(out), n_iter.value, bool(conv.value)


# ---------------------------------------------------------------- thin functional wrappers
def normalize_l1(m):
    check(load().hhx_normalize_l1(m.h))
    return m


def inflate(m, inflation):
    check(load().hhx_inflate(m.h, float(inflation)))
    return m


def prune(m, pruning):
    return DeviceCSR(new_handle('hhx_prune', m.h, float(pruning)))


def inflate_prune(c, inflation, pruning):
    return DeviceCSR(new_handle('hhx_inflate_prune', c.h, float(inflation), float(pruning)))


def inflate_prune_keep(c, inflation, pruning):
    return DeviceCSR(new_handle('hhx_inflate_prune_keep', c.h, float(inflation), float(pruning)))


def vstack(blocks):
    arr = (C.c_void_p * len(blocks))(*[b.h.value for b in blocks])
    return DeviceCSR(new_handle('hhx_csr_vstack', len(blocks), arr))


def mem_info():
    f, t = C.c_int64(0), C.c_int64(0)
    check(load().hhx_mem_info(C.byref(f), C.byref(t)))
    return f.value, t.value


def pool_prewarm(sizes):
    """hhx_pool_prewarm: blocks of these byte sizes from the driver into the pool's cache (call it from a helper thread while a long kernel runs)"""
    a = np.ascontiguousarray(sizes, np.int64)
    check(load().hhx_pool_prewarm(len(a), a.ctypes.data_as(c_i64p)))


def pool_cached_bytes():
    b = C.c_int64(0)
    check(load().hhx_pool_cached_bytes(C.byref(b)))
    return b.value


class DenseRows(Handle):
    """hhx_dense: rows [r0, r1) of the pre-expanded matrix M^2 as float32 in HBM — one expansion for a whole inflation sweep"""
    _release = 'hhx_dense_free'

    def __init__(self, links, r0, r1, fx_shift=52, upper_only=False):
        """upper_only: only the blocks (I, J >= I) of the rows are filled (integer arithmetic); the caller mirrors the rest"""
        self.h = C.c_void_p()
        f, z = C.c_int64(0), C.c_int64(0)
        check(load().hhx_expand_links_dense(links.h, int(r0), int(r1), int(fx_shift), int(bool(upper_only)), C.byref(self.h), C.byref(f), C.byref(z)))
        self.n_products, self.nnz_expanded = f.value, z.value
        self.n_rows, self.n_cols = int(r1) - int(r0), links.shape3[1]

    def device(self):
        """(device pointer of the block — n_rows rows of n_cols float32 —, row pitch in floats, columns per window, number of windows)"""
        x, ld, cap, nw = C.c_void_p(), C.c_int64(0), C.c_int32(0), C.c_int32(0)
        check(load().hhx_dense_device(self.h, C.byref(x), C.byref(ld), C.byref(cap), C.byref(nw)))
        return x.value or 0, ld.value, cap.value, nw.value

    def inflate_prune(self, inflation, pruning):
        """iteration 0 of mcl() (:2037-2042) of these rows at `inflation`"""
        return DeviceCSR(new_handle('hhx_dense_inflate_prune', self.h, float(inflation), float(pruning)))

    MULTI = 8       # inflations per pass of inflate_prune_multi (hhx_expand.hip: MULTI_MAX)

    def inflate_prune_multi(self, inflations, pruning):
        """iteration 0 at several inflations in one pass over the block per group of MULTI (hhx_dense_inflate_prune_multi): the
        matrices inflate_prune would return, in the order of `inflations`"""
        res = []
        inflations = [float(x) for x in inflations]
        for lo in range(0, len(inflations), self.MULTI):
            grp = inflations[lo:lo + self.MULTI]
            arr = (C.c_double * len(grp))(*grp)
            outs = (C.c_void_p * len(grp))()
            check(load().hhx_dense_inflate_prune_multi(self.h, len(grp), arr, float(pruning), outs))
            res.extend(DeviceCSR(o) for o in outs)
        return res


# ---------------------------------------------------------------- the pieces of the multi-rank driver (sharded.py): device addresses as ints
class ShardBuild(Handle):
    """hhx_shard: one rank's part of the sharded link-matrix build over `src`, its finalized Ingest"""
    _release = 'hhx_shard_destroy'

    def __init__(self, src, in_set):
        in_set = np.ascontiguousarray(in_set, np.uint8)
        self.n_frag = src.n_frag
        self.h = new_handle('hhx_shard_create', src.h, ptr(in_set))

    def first(self):
        """device address of the first positions, int64 [n_frag]"""
        p = C.c_void_p()
        check(load().hhx_shard_first(self.h, C.byref(p)))
        return p.value or 0

    def emit(self, fidx_ptr, bounds):
        """-> (w0, w1, counts): device addresses of the entries' two int64 words, ordered by owner, and the entries per owner (int64 array)"""
        b = np.ascontiguousarray(bounds, np.int32)
        counts = np.zeros(len(b) - 1, np.int64)
        w0, w1 = C.c_void_p(), C.c_void_p()
        check(load().hhx_shard_emit(self.h, C.c_void_p(fidx_ptr), len(b), b.ctypes.data_as(c_i32p), C.byref(w0), C.byref(w1),
                                    counts.ctypes.data_as(c_i64p)))
        return w0.value or 0, w1.value or 0, counts


def rank_first(n, first_ptr, fidx_ptr):
    """fills fidx (int32 [n]) from the first positions (int64 [n]); -> the number of linked fragments"""
    nl = C.c_int32(0)
    check(load().hhx_rank_first(int(n), C.c_void_p(first_ptr), C.c_void_p(fidx_ptr), C.byref(nl)))
    return nl.value


def rows_from_entries(n, w0_ptr, w1_ptr, r0, r1, shape):
    return DeviceCSR(new_handle('hhx_rows_from_entries', int(n), C.c_void_p(w0_ptr), C.c_void_p(w1_ptr), int(r0), int(r1), int(shape), 1))


def rows_from_runs(run_counts, w0_ptr, w1_ptr, r0, r1, shape):
    """rows_from_entries for entries that lie run after run (run_counts entries each), every run in row order already"""
    off = np.zeros(len(run_counts) + 1, np.int64)
    off[1:] = np.cumsum(run_counts)
    return DeviceCSR(new_handle('hhx_rows_from_runs', len(run_counts), off.ctypes.data_as(c_i64p), C.c_void_p(w0_ptr), C.c_void_p(w1_ptr), int(r0),
                                int(r1), int(shape), 1))


def csr_pack_block(m, buf_ptr, words):
    check(load().hhx_csr_pack_block(m.h, C.c_void_p(buf_ptr), int(words)))


def csr_unpack_blocks(rows, nnzs, packed_ptr, stride, n_cols):
    rows, nnzs = np.ascontiguousarray(rows, np.int64), np.ascontiguousarray(nnzs, np.int64)
    return DeviceCSR(new_handle('hhx_csr_unpack_blocks', len(rows), rows.ctypes.data_as(c_i64p), nnzs.ctypes.data_as(c_i64p), C.c_void_p(packed_ptr),
                                int(stride), int(n_cols)))


def transpose_f32(src_ptr, src_ld, dst_ptr, dst_ld, rows, cols):
    check(load().hhx_transpose_f32(C.c_void_p(src_ptr), int(src_ld), C.c_void_p(dst_ptr), int(dst_ld), int(rows), int(cols)))


def copy_rect_f32(src_ptr, src_ld, dst_ptr, dst_ld, rows, cols):
    check(load().hhx_copy_rect_f32(C.c_void_p(src_ptr), int(src_ld), C.c_void_p(dst_ptr), int(dst_ld), int(rows), int(cols)))


def links_integer_ok(links):
    """does iteration 0 on this raw link matrix run in the integer arithmetic (symmetric integer counts, row sums < 2^18)?"""
    ok, shift = C.c_int(0), C.c_int(0)
    check(load().hhx_links_integer_ok(links.h, C.byref(ok), C.byref(shift)))
    return bool(ok.value)


def links_plan(links):
    """(integer arithmetic?, layout of iteration 0: 0 all products into the fused epilogue / 1 square dense block / 2 upper block triangle)"""
    a, b = C.c_int(0), C.c_int(0)
    check(load().hhx_links_plan(links.h, C.byref(a), C.byref(b)))
    return bool(a.value), b.value


def mcl_resume(m, done, expansion, inflation, max_iter, pruning, want_stats=False):
    out = C.c_void_p()
    n_iter, conv = C.c_int(0), C.c_int(0)
    stats = np.zeros((max(int(max_iter), 1), 4), np.int64)
    check(load().hhx_mcl_resume(m.h, int(done), int(expansion), float(inflation), int(max_iter), float(pruning),
                                C.byref(out), C.byref(n_iter), C.byref(conv), ptr(stats)))
    res = (DeviceCSR(out), n_iter.value, bool(conv.value))
    return res + (stats[int(done):n_iter.value],) if want_stats else res


def spgemm(a, b, fx_shift=-1, want_products=False):
    out = C.c_void_p()
    f = C.c_int64(0)
    check(load().hhx_spgemm_ex(a.h, b.h, int(fx_shift), C.byref(out), C.byref(f) if want_products else None))
    return (DeviceCSR(out), f.value) if want_products else DeviceCSR(out)


def convergence_stat(m, last):
    s = C.c_float(0)
    check(load().hhx_convergence_stat(m.h, last.h, C.byref(s)))
    return s.value


def expand_inflate_prune(a, b, inflation, pruning, fx_shift=52):
    """one fused iteration: prune(normalize(power(a*b, r))); returns (matrix, n_products, nnz_expanded)"""
    out = C.c_void_p()
    f, z = C.c_int64(0), C.c_int64(0)
    check(load().hhx_expand_inflate_prune(a.h, b.h, int(fx_shift), float(inflation), float(pruning), C.byref(out),
                                          C.byref(f), C.byref(z)))
    return DeviceCSR(out), f.value, z.value


def link_weights(frag_i, frag_j, value, mode, n_frag, per_frag=None, tag=None, param=0.0, device_ptrs=None):
    """hhx_link_weights on host arrays (value: float64, rewritten in place) or, with device_ptrs = (i, j, value) device
    addresses of n = len(...) keys, on the device arrays of hhx_ingest_flank_device.  Returns the number of zeroed entries."""
    nz = C.c_int64(0)
    per = None if per_frag is None else np.ascontiguousarray(per_frag, np.int64)
    tg = None if tag is None else np.ascontiguousarray(tag, np.int32)
    if device_ptrs is not None:
        n, pi, pj, pv = device_ptrs
        check(load().hhx_link_weights(int(n), C.c_void_p(pi), C.c_void_p(pj), C.c_void_p(pv), 1, int(mode), int(n_frag), ptr(per), ptr(tg),
                                      float(param), C.byref(nz)))
        return nz.value
    assert value.dtype == np.float64 and value.flags.c_contiguous
    fi, fj = np.ascontiguousarray(frag_i, np.int32), np.ascontiguousarray(frag_j, np.int32)
    check(load().hhx_link_weights(len(value), ptr(fi), ptr(fj), ptr(value), 0, int(mode), int(n_frag), ptr(per), ptr(tg), float(param),
                                  C.byref(nz)))
    return nz.value


def names_blob(names, encode=str.encode):
    """names -> (uint8 array of the UTF-8 bytes back to back, int64 offsets [len(names) + 1]); encode: os.fsencode for paths"""
    enc = [encode(n) for n in names]
    off = np.zeros(len(enc) + 1, np.int64)
    if enc:
        np.cumsum(np.fromiter(map(len, enc), np.int64, len(enc)), out=off[1:])
    blob = np.frombuffer(b''.join(enc) or b'\0', np.uint8)
    return blob, off


def write_link_pickle(path, i, j, count, names):
    """full_links.pkl / HT_links.pkl (output_pickle :710-715) straight from the link arrays: a protocol-4 pickle of
    `defaultdict(int)` {(names[i[k]], names[j[k]]): count[k]} in array order, written by the library's host code
    (hhx_write_link_pickle) without a Python object per key.  Returns the bytes written."""
    fi, fj = np.ascontiguousarray(i, np.int32), np.ascontiguousarray(j, np.int32)
    cnt = np.ascontiguousarray(count, np.int64)
    blob, off = names_blob(names)
    n_bytes = C.c_int64(0)
    check(load().hhx_write_link_pickle(os.fsencode(path), fi.size, ptr(fi), ptr(fj), ptr(cnt), len(names), ptr(blob), ptr(off),
                                       C.byref(n_bytes)))
    return n_bytes.value


PICKLE_NOT_OURS = HHX_UNSUPPORTED
PICKLE_REFUSALS = []                 # hhx_last_error() of every file read_link_pickle handed back in this process


class LinkPickle(Handle):
    """hhx_pickle: full_links.pkl / HT_links.pkl read into arrays that stay in the memory of the device (hhx_pickle_open) until close().
    LinkPickle.open(path) -> the handle, or None for a file the reader does not answer (the reason goes to PICKLE_REFUSALS; the caller runs
    pickle.load).  tests/sort_heads_cases.py holds a host engine with the same interface."""
    _release = 'hhx_pickle_free'

    def __init__(self, h):
        self.h = h
        n_keys, n_names, n_bytes, any_float = C.c_int64(0), C.c_int32(0), C.c_int64(0), C.c_int(0)
        check(load().hhx_pickle_sizes(h, C.byref(n_keys), C.byref(n_names), C.byref(n_bytes), C.byref(any_float)))
        self.n_keys, self.n_names, self.names_bytes, self.any_float = n_keys.value, n_names.value, n_bytes.value, bool(any_float.value)

    @classmethod
    def open(cls, path):
        h = C.c_void_p()
        if not check_served(load().hhx_pickle_open(os.fsencode(path), C.byref(h))):
            PICKLE_REFUSALS.append(last_error())
            return None
        return cls(h)                   # (released by the finaliser if the sizes cannot be read)

    def _decode(self, blob, off):
        text, bounds = blob.tobytes(), off.tolist()
        return [text[a:b].decode() for a, b in zip(bounds[:-1], bounds[1:])]

    def names(self):
        """the distinct names in order of first appearance (the names alone: the keys stay on the device); UnicodeDecodeError for a name that is
        not UTF-8"""
        blob, off = np.empty(max(1, self.names_bytes), np.uint8), np.empty(self.n_names + 1, np.int64)
        check(load().hhx_pickle_fetch(self.h, None, None, None, None, ptr(blob), ptr(off)))
        return self._decode(blob, off)

    def arrays(self):
        """(i, j, value, is_float, names) as read_link_pickle returns them, or None where it returns None"""
        i, j = np.empty(self.n_keys, np.int32), np.empty(self.n_keys, np.int32)
        value, is_float = np.empty(self.n_keys, np.int64), np.empty(self.n_keys, np.uint8)
        blob, off = np.empty(max(1, self.names_bytes), np.uint8), np.empty(self.n_names + 1, np.int64)
        check(load().hhx_pickle_fetch(self.h, ptr(i), ptr(j), ptr(value), ptr(is_float), ptr(blob), ptr(off)))
        try:
            names = self._decode(blob, off)
        except UnicodeDecodeError as e:                                           # pickle.load raises its own error for such a name
            PICKLE_REFUSALS.append('a name is not UTF-8: %s' % e)
            return None
        if not self.any_float:
            return i, j, value, None, names
        is_float = is_float.astype(bool)
        out = value.view(np.float64).copy()
        ints = value[~is_float]
        if ((ints > 2 ** 53) | (ints < -2 ** 53)).any():
            PICKLE_REFUSALS.append('integers beyond 2^53 beside floats')
            return None
        out[~is_float] = ints
        return i, j, out, is_float, names

    def group_heads(self, n_ctg, slot, rank):
        """hhx_pickle_group_heads: get_sub_HT_dict :117-143 for one group -> (ei, ej, w): int32 index pairs and int64 values in the reference's
        insertion order.  slot [n_names] and rank [n_ctg] as include/haphic_hip.h describes them."""
        slot, rank = np.ascontiguousarray(slot, np.int32), np.ascontiguousarray(rank, np.int32)
        if slot.size != self.n_names or rank.size != n_ctg:
            raise ValueError('LinkPickle.group_heads: {} slots for {} names, {} ranks for {} contigs'.format(slot.size, self.n_names, rank.size, n_ctg))
        n = C.c_int64(0)
        check(load().hhx_pickle_group_heads(self.h, int(n_ctg), ptr(slot), ptr(rank), C.byref(n)))
        ei, ej, w = np.empty(n.value, np.int32), np.empty(n.value, np.int32), np.empty(n.value, np.int64)
        if n.value:
            check(load().hhx_pickle_group_heads_fetch(self.h, ptr(ei), ptr(ej), ptr(w)))
        return ei, ej, w


def read_link_pickle(path):
    """full_links.pkl / HT_links.pkl -> (i, j, value, is_float, names) in dict insertion order, without a Python object per key (hhx_pickle_open):
    int32 ids into `names` (distinct names in order of first appearance, i before j, key by key), value int64 with is_float None when every
    value is an integer, else float64 with a bool array saying which keys hold a float.  None: not a file this reader answers (the header lists
    what that is; the reason goes to PICKLE_REFUSALS) — the caller runs pickle.load.  Integers beyond 2^53 beside floats are handed back too:
    float64 would not hold them."""
    h = LinkPickle.open(path)
    if h is None:
        return None
    try:
        return h.arrays()
    finally:
        h.close()


# ---- the file-writer thread of the library (hhx_jobs.hip): output_pickle / output_clm return at once, the files are complete after files_join()
_pending_arrays = []                 # arrays of hhx_write_link_pickle_async that the library reads until the join
_join_registered = False


def files_async():
    """False: HAPHIC_SYNC_FILES=1 in the environment — the writers run on the caller's thread as they did before round 6"""
    return os.environ.get('HAPHIC_SYNC_FILES', '') not in ('1', 'true', 'yes')


def _register_join():
    global _join_registered
    if not _join_registered:
        import atexit
        atexit.register(_join_at_exit)
        _join_registered = True


def _join_at_exit():
    try:
        files_join()
    except RuntimeError as e:        # nobody is left to catch it: say it where a user sees it
        import sys
        print('haphic_amd: a file queued by output_pickle / output_clm was not written: %s' % e, file=sys.stderr)


def files_pending():
    """(files queued or being written, files finished since the library was loaded)"""
    a, b = C.c_int64(0), C.c_int64(0)
    check(load().hhx_files_pending(C.byref(a), C.byref(b)))
    return a.value, b.value


def files_join():
    """wait for every queued file (hhx_files_join); RuntimeError with the first failure if a writer failed"""
    if _lib is None:
        return
    n = C.c_int64(0)
    rc = _lib.hhx_files_join(C.byref(n))
    del _pending_arrays[:]
    check(rc)


class ByteSink(Handle):
    """hhx_byte_sink: a file fed from device buffers through the library's file-writer thread (alignments.bed, deferred).
    The one handle whose close() is an action with a result — it queues the file's close, returns the bytes handed over and raises when that
    failed — so it is never closed behind the caller's back: `with` closes it, the finaliser does not (closing a half-fed or never-based deferred
    sink from the garbage collector would change what reaches the disk)."""
    _release = 'hhx_byte_sink_close'
    _finalise = False

    def __init__(self, path, hbm_budget_bytes=0, expected_bytes=0, deferred=False):
        """deferred: the bytes go to the file at an offset given later by set_base() (hhx_byte_sink_open_deferred)"""
        _register_join()
        self.h = new_handle('hhx_byte_sink_open_deferred' if deferred else 'hhx_byte_sink_open', os.fsencode(path), int(hbm_budget_bytes),
                            int(expected_bytes))

    def set_base(self, base):
        check(load().hhx_byte_sink_set_base(self.h, int(base)))

    def close(self):
        """queue the close (the file is complete after files_join()); returns the bytes handed to the sink"""
        n = C.c_int64(0)
        if getattr(self, 'h', None):
            check(load().hhx_byte_sink_close(self.h, C.byref(n)))
        self.h = None
        return n.value


class TextReader(Handle):
    """hhx_text_reader: a text file as chunks of whole lines in pinned host memory, read ahead by threads of the library"""
    _release = 'hhx_text_reader_close'

    def __init__(self, path, chunk_bytes=256 << 20, threads=4, bgzf=False, byte_range=None):
        """bgzf: the file is bgzipped (BGZF blocks inflated by the threads); RuntimeError('... is not a BGZF file ...') for anything else.
        byte_range (begin, end): only the lines whose first byte lies in it (hhx_text_reader_open_range; BGZF: compressed offsets)"""
        if byte_range is not None:
            self.h = new_handle('hhx_text_reader_open_range', os.fsencode(path), int(byte_range[0]), int(byte_range[1]), int(chunk_bytes), int(threads),
                                int(bool(bgzf)))
            return
        self.h = new_handle('hhx_text_reader_open_bgzf' if bgzf else 'hhx_text_reader_open', os.fsencode(path), int(chunk_bytes), int(threads))

    def __iter__(self):
        """(host pointer, bytes) per chunk; a pointer is valid until the next one is asked for"""
        host, n = C.c_void_p(), C.c_int64(0)
        while True:
            check(load().hhx_text_reader_next(self.h, C.byref(host), C.byref(n)))
            if n.value == 0:
                return
            yield host.value, n.value


class ClmSplit(Handle):
    """hhx_clm_split: CLM text, pushed in pieces cut anywhere, routed line by line to one file per group (split_clm_file,
    HapHiC_reassign.py:581-622).  names[k] belongs to group group_of_name[k] (-1: to none); paths[g] is the file of group g."""
    STATS = ('lines', 'kept', 'heads', 'seams', 'continuations', 'multi_line_tiles', 'multi_tile_lines')
    _release = 'hhx_clm_split_destroy'

    def __init__(self, names, group_of_name, paths):
        blob, off = names_blob(names)
        grp = np.ascontiguousarray(group_of_name, np.int32)
        if grp.size != len(names):
            raise ValueError('ClmSplit: {} names, {} groups of names'.format(len(names), grp.size))
        pblob, poff = names_blob(paths, os.fsencode)
        self.n_groups = len(poff) - 1
        self.h = new_handle('hhx_clm_split_create', len(names), ptr(blob), ptr(off), ptr(grp) if grp.size else None, self.n_groups, ptr(pblob), ptr(poff))

    def push(self, text=None, device_ptr=None, n_bytes=None):
        """the next bytes of the file: bytes-like, or a device pointer + n_bytes; IndexError as the reference's cols[1] raises it"""
        if device_ptr is not None:
            return check_py(load().hhx_clm_split_push(self.h, C.c_void_p(device_ptr), int(n_bytes), 1))
        buf = np.frombuffer(text, np.uint8)
        check_py(load().hhx_clm_split_push(self.h, ptr(buf) if buf.size else None, buf.size, 0))

    def push_file(self, path, chunk_bytes=64 << 20, threads=4):
        """the whole file through the library's pinned read-ahead reader, in raw chunks of chunk_bytes"""
        check_py(load().hhx_clm_split_file(self.h, os.fsencode(path), int(chunk_bytes), int(threads)))

    def finish(self):
        """flushes the open line; the files are complete on return.  -> (lines, lines kept, bytes per group)"""
        nl, nk = C.c_int64(0), C.c_int64(0)
        per = np.zeros(max(self.n_groups, 1), np.int64)
        check_py(load().hhx_clm_split_finish(self.h, C.byref(nl), C.byref(nk), ptr(per)))
        return nl.value, nk.value, per[:self.n_groups]

    def stats(self):
        v = np.zeros(len(self.STATS), np.int64)
        check(load().hhx_clm_split_stats(self.h, ptr(v)))
        return dict(zip(self.STATS, (int(x) for x in v)))


class SortGraph(Handle):
    """hhx_sort_graph: the dense work of one group of `haphic sort`'s fast sorting (HapHiC_sort.py :60-88 :158-244 :406-435 :456-467), per round.
    Built from the round-1 edges (index pairs, integer weights); tests/sort_cases.py holds a numpy engine with the same interface."""
    METHODS = {'sum': 0, 'multiplication': 1, 'geometric_mean': 2}
    STATS = ('lds_aggregations', 'global_aggregations', 'cells_over', 'pairs_flagged')
    FOREST_STATS = ('lds_forests', 'hbm_forests', 'boruvka_rounds', 'jump_rounds', 'confidence_copies')
    _release = 'hhx_sort_graph_destroy'

    def __init__(self, shape, ei, ej, w):
        ei, ej = np.ascontiguousarray(ei, np.int32), np.ascontiguousarray(ej, np.int32)
        w = np.ascontiguousarray(w, np.int64)
        if not (ei.size == ej.size == w.size):
            raise ValueError('SortGraph: {} / {} indices, {} weights'.format(ei.size, ej.size, w.size))
        self.h = new_handle('hhx_sort_graph_create', int(shape), ei.size, ptr(ei) if ei.size else None, ptr(ej) if ei.size else None,
                            ptr(w) if ei.size else None)

    @property
    def shape(self):
        n = C.c_int32(0)
        check(load().hhx_sort_graph_shape(self.h, C.byref(n), None, None))
        return n.value

    def density(self, lengths, method):
        """D = S / L on the device -> the flagged geometric-mean pairs as an (n, 2) int32 array (usually empty) for patch_len"""
        ln = np.ascontiguousarray(lengths, np.float64)
        if ln.size != self.shape:
            raise ValueError('SortGraph.density: {} lengths for shape {}'.format(ln.size, self.shape))
        n = C.c_int64(0)
        check(load().hhx_sort_graph_density(self.h, ptr(ln), self.METHODS[method] if isinstance(method, str) else int(method), C.byref(n)))
        pairs = np.empty((n.value, 2), np.int32)
        if n.value:
            check(load().hhx_sort_graph_fetch_flagged(self.h, ptr(pairs)))
        return pairs

    def patch_len(self, pairs, L):
        pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
        pi, pj = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
        L = np.ascontiguousarray(L, np.float32)
        check(load().hhx_sort_graph_patch_len(self.h, pi.size, ptr(pi), ptr(pj), ptr(L)))

    def confidence(self, pair_a, pair_b):
        """-> (float64 array shape x shape, MAXS as numpy.float64); the array is a view of the one buffer the device copy filled"""
        pa, pb = np.ascontiguousarray(pair_a, np.int32), np.ascontiguousarray(pair_b, np.int32)
        n = self.shape
        buf = np.empty(n * n + 1, np.float64)
        check(load().hhx_sort_graph_confidence(self.h, pa.size, ptr(pa) if pa.size else None, ptr(pb) if pb.size else None, ptr(buf)))
        return buf[:n * n].reshape(n, n), buf[n * n]

    def confidence_device(self, pair_a, pair_b):
        """confidence() without the copy: the array stays on the device (forest, fetch_confidence) -> MAXS as numpy.float64"""
        pa, pb = np.ascontiguousarray(pair_a, np.int32), np.ascontiguousarray(pair_b, np.int32)
        maxs = np.empty(1, np.float64)
        check(load().hhx_sort_graph_confidence_device(self.h, pa.size, ptr(pa) if pa.size else None, ptr(pb) if pb.size else None, ptr(maxs)))
        return maxs[0]

    def fetch_confidence(self):
        """the confidence array as it is on the device now (filtered, once forest() ran)"""
        n = self.shape
        out = np.empty((n, n), np.float64)
        check(load().hhx_sort_graph_fetch_confidence(self.h, ptr(out)))
        return out

    def forest(self, cutoff):
        """filter_confidence_graph + the maximum spanning forest of networkx's Kruskal on the device -> (eu, ev, label, pos, not_paths): the chosen
        edges (u < v) in Kruskal's order, the smallest index of every node's tree, the position along its path from the smaller-index end (-1
        everywhere when not_paths: some node has no edge or more than two)"""
        nch, bad = C.c_int64(0), C.c_int32(0)
        check(load().hhx_sort_graph_forest(self.h, float(cutoff), C.byref(nch), C.byref(bad)))
        n = self.shape
        eu, ev, label, pos = np.empty(nch.value, np.int32), np.empty(nch.value, np.int32), np.empty(n, np.int32), np.empty(n, np.int32)
        check(load().hhx_sort_graph_fetch_forest(self.h, ptr(eu) if nch.value else None, ptr(ev) if nch.value else None, ptr(label), ptr(pos)))
        return eu, ev, label, pos, bool(bad.value)

    def forest_stats(self):
        v = np.zeros(len(self.FOREST_STATS), np.int64)
        check(load().hhx_sort_graph_forest_stats(self.h, ptr(v)))
        return dict(zip(self.FOREST_STATS, (int(x) for x in v)))

    def drop(self, a, b):
        check(load().hhx_sort_graph_drop(self.h, int(a), int(b)))

    def aggregate(self, new_shape, index_map):
        """-> (i, j, w, cells_over): the new edges (i > j, row-major, float32 values) and the positions i * new_shape + j of the cells above 2^24"""
        m = np.ascontiguousarray(index_map, np.int32)
        ne, no = C.c_int64(0), C.c_int64(0)
        check(load().hhx_sort_graph_aggregate(self.h, int(new_shape), ptr(m), C.byref(ne), C.byref(no)))
        ei, ej, w = np.empty(ne.value, np.int32), np.empty(ne.value, np.int32), np.empty(ne.value, np.float32)
        check(load().hhx_sort_graph_fetch_edges(self.h, ptr(ei), ptr(ej), ptr(w)))
        over = np.empty(no.value, np.int64)
        if no.value:
            check(load().hhx_sort_graph_fetch_over(self.h, ptr(over)))
            over.sort()
        return ei, ej, w, over

    def patch_cells(self, cells, ordinal, values):
        c, o = np.ascontiguousarray(cells, np.int64), np.ascontiguousarray(ordinal, np.int64)
        v = np.ascontiguousarray(values, np.float32)
        check(load().hhx_sort_graph_patch_cells(self.h, c.size, ptr(c), ptr(o), ptr(v)))

    def matrix(self):
        return self._dense(0)

    def density_graph(self):
        return self._dense(1)

    def _dense(self, which):
        n = self.shape
        out = np.empty((n, n), np.float32)
        check(load().hhx_sort_graph_fetch_dense(self.h, which, ptr(out)))
        return out

    def stats(self):
        v = np.zeros(len(self.STATS), np.int64)
        check(load().hhx_sort_graph_stats(self.h, ptr(v)))
        return dict(zip(self.STATS, (int(x) for x in v)))


class SortVerdictUnsupported(RuntimeError):
    """hhx_sort_verdict_sums answered HHX_UNSUPPORTED: the caller takes the reference's function"""


SORT_VERDICT_STATS = ('lds_rotations', 'hbm_rotations', 'cell_bytes')


def sort_verdict_sums(value, lengths, r0=0, r1=None, want_stats=False):
    """hhx_sort_verdict_sums: the weighted-LIS sums s[r0 .. r1) of compare_fast_sort_and_allhic (HapHiC_sort.py :696-721) as int64; value[i] = +-(pos + 1)
    of element i of the fast-sort tour, lengths[i] its contig length; r1 None: n - 1, every rotation the reference looks at.  want_stats: (sums, dict
    of SORT_VERDICT_STATS).  tests/sort_verdict_cases.py holds a host engine with the same signature.  Raises SortVerdictUnsupported where the library
    answers HHX_UNSUPPORTED."""
    v, ln = np.ascontiguousarray(value, np.int32), np.ascontiguousarray(lengths, np.int64)
    if v.ndim != 1 or v.shape != ln.shape:
        raise ValueError('sort_verdict_sums: {} values, {} lengths'.format(v.shape, ln.shape))
    n = int(v.size)
    r1 = n - 1 if r1 is None else int(r1)
    sums = np.zeros(max(r1 - int(r0), 0), np.int64)
    stats = np.zeros(len(SORT_VERDICT_STATS), np.int64)
    rc = load().hhx_sort_verdict_sums(n, ptr(v), ptr(ln), int(r0), r1, ptr(sums), ptr(stats))
    check_served(rc, SortVerdictUnsupported)
    return (sums, dict(zip(SORT_VERDICT_STATS, (int(x) for x in stats)))) if want_stats else sums


def write_link_pickle_async(path, i, j, count, names):
    """write_link_pickle on the library's file-writer thread; the arrays are kept alive here until files_join()"""
    fi, fj = np.ascontiguousarray(i, np.int32), np.ascontiguousarray(j, np.int32)
    cnt = np.ascontiguousarray(count, np.int64)
    blob, off = names_blob(names)
    _register_join()
    _pending_arrays.append((fi, fj, cnt))
    check(load().hhx_write_link_pickle_async(os.fsencode(path), fi.size, ptr(fi), ptr(fj), ptr(cnt), len(names), ptr(blob), ptr(off)))


def group_link_sums(frag_i, frag_j, links, group, n_groups):
    """hhx_group_link_sums: (sums, first) int64 [n_ctg, n_groups]; first == -1 where a cell got no contribution"""
    fi, fj = np.ascontiguousarray(frag_i, np.int32), np.ascontiguousarray(frag_j, np.int32)
    lk = np.ascontiguousarray(links, np.int64)
    grp = np.ascontiguousarray(group, np.int32)
    sums = np.zeros((len(grp), int(n_groups)), np.int64)
    first = np.full((len(grp), int(n_groups)), -1, np.int64)
    check(load().hhx_group_link_sums(len(lk), ptr(fi), ptr(fj), ptr(lk), len(grp), ptr(grp), int(n_groups), ptr(sums), ptr(first)))
    return sums, first


def _group_stats_args(group, n_groups, group_re, ctg_re):
    grp = np.ascontiguousarray(group, np.int32)
    if grp.ndim != 2:
        raise ValueError('group_stats: group is [n_sets, n_ctg]')
    ng = np.ascontiguousarray(n_groups, np.int32)
    gre, cre = np.ascontiguousarray(group_re, np.int64), np.ascontiguousarray(ctg_re, np.int64)
    if ng.shape != (grp.shape[0],) or cre.shape != (grp.shape[1],) or gre.shape != (int(ng.sum()),):
        raise ValueError('group_stats: n_groups per set, group_re for all groups of all sets, ctg_re per contig')
    out = (np.zeros(grp.shape, np.int32), np.zeros(grp.shape, np.int64), np.full(grp.shape, -1, np.int32), np.zeros(grp.shape, np.float64))
    return grp, ng, gre, cre, out


GROUP_STATS_UNSUPPORTED = HHX_UNSUPPORTED


def group_stats(frag_i, frag_j, links, group, n_groups, group_re, ctg_re, sum_mode=0):
    """hhx_group_stats — what output_statistics :2279-2478 keeps of ctg_group_link_dict, for every set (group assignment) at once: keys
    (frag_i, frag_j, links) in dict order, group int32 [n_sets, n_ctg] (-1 = ungrouped), n_groups [n_sets], group_re = the sets' group_RE values
    one set after the other, ctg_re [n_ctg].  Returns (n_cells, max_links, max_group, other_sum), each [n_sets, n_ctg] (include/haphic_hip.h),
    or None when the library does not serve the call.  sum_mode 0: plain sum, 1: CPython >= 3.12's compensated sum()."""
    fi, fj = np.ascontiguousarray(frag_i, np.int32), np.ascontiguousarray(frag_j, np.int32)
    lk = np.ascontiguousarray(links, np.int64)
    grp, ng, gre, cre, out = _group_stats_args(group, n_groups, group_re, ctg_re)
    rc = load().hhx_group_stats(len(lk), ptr(fi), ptr(fj), ptr(lk), 0, grp.shape[1], grp.shape[0], ptr(grp), ptr(ng), ptr(gre), ptr(cre), int(sum_mode),
                                *[ptr(a) for a in out])
    return out if check_served(rc) else None


class Reassign(Handle):
    """hhx_reassign: the cells, the adjacency and the keys of one full_link_dict in HBM for the rounds of `haphic reassign` (run_reassignment
    :266-427) and the group-pair sums of its agglomerative step (include/haphic_hip.h).  tests/reassign_cases.py holds a numpy engine with the
    same interface.  Raises Unsupported where the library answers HHX_UNSUPPORTED."""
    _release = 'hhx_reassign_destroy'

    class Unsupported(RuntimeError):
        pass

    REFUSALS = []                       # (flags, hhx_last_error()) of every table from_pickle handed back in this process
    REFUSED_SELF_KEY, REFUSED_FLOAT, REFUSED_NEGATIVE, REFUSED_TOTAL, REFUSED_KEYS = 1, 2, 4, 8, 16    # HHX_REFUSED_*

    def __init__(self, frag_i, frag_j, links, n_ctg, group, n_groups):
        fi, fj = np.ascontiguousarray(frag_i, np.int32), np.ascontiguousarray(frag_j, np.int32)
        lk, grp = np.ascontiguousarray(links, np.int64), np.ascontiguousarray(group, np.int32)
        if not (fi.size == fj.size == lk.size) or grp.size != int(n_ctg):
            raise ValueError('Reassign: {} / {} / {} key arrays, {} groups for {} contigs'.format(fi.size, fj.size, lk.size, grp.size, n_ctg))
        self.n_ctg, self.n_groups = int(n_ctg), int(n_groups)
        self.rounds = 0                 # device rounds so far: the tables are the reference's dicts only while it is 0
        self.launches = 0               # launch pairs of the last round
        self.h = C.c_void_p()
        rc = load().hhx_reassign_create(fi.size, ptr(fi), ptr(fj), ptr(lk), self.n_ctg, ptr(grp), self.n_groups, C.byref(self.h))
        check_served(rc, Reassign.Unsupported)

    @classmethod
    def from_pickle(cls, link_pickle, n_ctg, group, n_groups):
        """the handle from the keys of an open LinkPickle where they lie in HBM (hhx_reassign_create_from_pickle): ids = the pickle's name ids,
        n_ctg >= its name count.  -> a Reassign, or None when the pass over the keys finds what the host path has to answer (a key naming one contig
        twice, a float or negative value, totals reaching 2^52, 2^31 keys); the reason goes to REFUSALS.  Unsupported: the cells of n_ctg x n_groups
        beyond half of the device's memory, as for Reassign(...)"""
        grp = np.ascontiguousarray(group, np.int32)
        if grp.size != int(n_ctg) or int(n_ctg) < link_pickle.n_names:
            raise ValueError('Reassign.from_pickle: {} groups for {} contigs, {} names in the table'.format(grp.size, n_ctg, link_pickle.n_names))
        self = cls.__new__(cls)
        self.n_ctg, self.n_groups = int(n_ctg), int(n_groups)
        self.rounds = self.launches = 0
        self.h = C.c_void_p()
        refused = C.c_int(0)
        rc = load().hhx_reassign_create_from_pickle(link_pickle.h, self.n_ctg, ptr(grp), self.n_groups, C.byref(refused), C.byref(self.h))
        check_served(rc, Reassign.Unsupported)
        if refused.value:
            cls.REFUSALS.append((refused.value, last_error()))
            return None
        return self

    def cells(self):
        """(sums, first) int64 [n_ctg, n_groups] as group_link_sums returns them"""
        sums, first = np.zeros((self.n_ctg, self.n_groups), np.int64), np.full((self.n_ctg, self.n_groups), -1, np.int64)
        check(load().hhx_reassign_cells(self.h, ptr(sums), ptr(first)))
        return sums, first

    def round(self, group, group_re, ctg_re, order, flags, dismissed, min_links, min_link_density, min_density_ratio, ambiguous_cutoff,
              is_rescue_round, gfa, sum_mode):
        """one call of run_reassignment: group (int32 [n_ctg], -1 = 'ungrouped') and group_re (int64 [n_groups]) are changed in place;
        -> counts int64 [4] (consistent, rescued, reassigned, not rescued)"""
        for a, dt, n in ((group, np.int32, self.n_ctg), (group_re, np.int64, self.n_groups)):
            if not (isinstance(a, np.ndarray) and a.dtype == dt and a.flags.c_contiguous and a.shape == (n,)):
                raise ValueError('Reassign.round: group is a contiguous int32 [n_ctg] array, group_re an int64 [n_groups] one (changed in place)')
        cre, od = np.ascontiguousarray(ctg_re, np.int64), np.ascontiguousarray(order, np.int32)
        fl = np.ascontiguousarray(flags, np.uint8)
        dm = None if dismissed is None else np.ascontiguousarray(dismissed, np.uint8)
        if cre.shape != (self.n_ctg,) or fl.shape != (self.n_ctg,) or (dm is not None and dm.shape != (self.n_groups,)):
            raise ValueError('Reassign.round: ctg_re and flags per contig, dismissed per group')
        counts, launches = np.zeros(4, np.int64), C.c_int64(0)
        rc = load().hhx_reassign_round(self.h, ptr(group), ptr(group_re), ptr(cre), od.size, ptr(od), ptr(fl), ptr(dm), float(min_links),
                                       float(min_link_density), float(min_density_ratio), float(ambiguous_cutoff), int(bool(is_rescue_round)),
                                       int(bool(gfa)), int(sum_mode), ptr(counts), C.byref(launches))
        check_served(rc, Reassign.Unsupported)
        self.rounds += 1
        self.launches = launches.value
        return counts

    def pair_sums(self, member, group_of_ctg, n_groups):
        """(sums, first) int64 [n_groups, n_groups]: the links between the member contigs of two different groups at cell (smaller id, larger id)
        and the dict position of the first such key (-1 = none)"""
        mb, grp = np.ascontiguousarray(member, np.uint8), np.ascontiguousarray(group_of_ctg, np.int32)
        if mb.shape != (self.n_ctg,) or grp.shape != (self.n_ctg,):
            raise ValueError('Reassign.pair_sums: member and group_of_ctg per contig')
        sums, first = np.zeros((int(n_groups), int(n_groups)), np.int64), np.full((int(n_groups), int(n_groups)), -1, np.int64)
        check(load().hhx_reassign_pair_sums(self.h, ptr(mb), ptr(grp), int(n_groups), ptr(sums), ptr(first)))
        return sums, first


class Fasta(Handle):
    """hhx_fasta: one FASTA file parsed on the device (parse_fasta, HapHiC_cluster.py:87-113) — the sequences back to back in HBM, the table on the
    host — and the writer of scaffolds.fa over it (build_final_scaffolds, HapHiC_build.py:153-168).  source: a path (str / os.PathLike) or the bytes
    of the file.  tests/build_cases.py holds a numpy engine with the same interface.  Raises Unsupported where the library answers HHX_UNSUPPORTED."""
    _release = 'hhx_fasta_close'

    class Unsupported(RuntimeError):
        pass

    def __init__(self, source, keep_letter_case=False):
        self.h = C.c_void_p()
        if isinstance(source, (str, os.PathLike)):
            rc = load().hhx_fasta_open(os.fsencode(source), int(bool(keep_letter_case)), C.byref(self.h))
        else:
            buf = np.frombuffer(source, np.uint8)
            rc = load().hhx_fasta_open_bytes(ptr(buf) if buf.size else None, buf.size, int(bool(keep_letter_case)), C.byref(self.h))
        check_served(rc, Fasta.Unsupported)
        n, ns, nn = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(load().hhx_fasta_counts(self.h, C.byref(n), C.byref(ns), C.byref(nn)))
        self.n_ctg, self.n_seq_bytes = n.value, ns.value
        self.seq_off, self.seq_len = np.zeros(self.n_ctg, np.int64), np.zeros(self.n_ctg, np.int64)
        self.name_off, self.name_bytes = np.zeros(self.n_ctg + 1, np.int64), np.zeros(max(nn.value, 1), np.uint8)
        check(load().hhx_fasta_table(self.h, ptr(self.seq_off), ptr(self.seq_len), ptr(self.name_off), ptr(self.name_bytes)))
        self.name_bytes = self.name_bytes[:nn.value]

    def names(self):
        """the contig names in file order (the text is ASCII: a byte >= 0x80 is refused)"""
        blob, off = self.name_bytes.tobytes().decode('ascii'), self.name_off.tolist()
        return [blob[off[k]:off[k + 1]] for k in range(self.n_ctg)]

    def sequences(self):
        """the sequences of all contigs, one after the other (uint8; contig k: [seq_off[k], seq_off[k] + seq_len[k]))"""
        out = np.zeros(max(self.n_seq_bytes, 1), np.uint8)
        check(load().hhx_fasta_sequences(self.h, ptr(out)))
        return out[:self.n_seq_bytes]

    def re_counts(self, sites):
        """occurrences of the (N-expanded, bytes) sites per contig, int64 (count_RE_sites :75-84)"""
        return count_re_sites(self.sequences(), self.seq_off, self.seq_len, sites)

    def re_counts_device(self, sites, seg_off=None, seg_len=None):
        """re_counts on the sequences where they lie in HBM (hhx_fasta_re_counts): no sequence byte is copied.  Segments in the handle's sequence
        coordinates; by default the whole contigs"""
        off = np.ascontiguousarray(self.seq_off if seg_off is None else seg_off, np.int64)
        ln = np.ascontiguousarray(self.seq_len if seg_len is None else seg_len, np.int64)
        if off.shape != ln.shape or off.ndim != 1:
            raise ValueError('Fasta.re_counts_device: {} offsets, {} lengths'.format(off.shape, ln.shape))
        pats = np.frombuffer(b''.join(sites), np.uint8) if sites else np.zeros(1, np.uint8)
        plen = np.array([len(x) for x in sites], np.int32) if sites else np.zeros(1, np.int32)
        out = np.zeros(max(off.size, 1), np.int64)
        check(load().hhx_fasta_re_counts(self.h, off.size, ptr(off), ptr(ln), len(sites), ptr(pats), ptr(plen), ptr(out)))
        return out[:off.size]

    def fetch(self, off, len):
        """bytes [off, off + len) of the resident sequences (hhx_fasta_fetch); a range outside them raises"""
        out = np.zeros(max(min(int(len), self.n_seq_bytes), 1), np.uint8)        # (a longer range is refused before a byte is written)
        check(load().hhx_fasta_fetch(self.h, int(off), int(len), ptr(out)))
        return out[:max(int(len), 0)].tobytes()

    def emit(self, path, rec_names, piece_off, piece_ctg, piece_rev, Ns, max_width):
        """writes the records (rec_names: list of str; record r: pieces [piece_off[r], piece_off[r + 1]) = (contig id, reversed?)) as a FASTA file
        of max_width columns, pieces joined by Ns 'N'.  -> bytes written"""
        blob, off = names_blob(rec_names)
        po, pc = np.ascontiguousarray(piece_off, np.int64), np.ascontiguousarray(piece_ctg, np.int32)
        pr = np.ascontiguousarray(piece_rev, np.uint8)
        if po.size != len(rec_names) + 1 or pc.size != pr.size or (po.size and pc.size != po[-1]):
            raise ValueError('Fasta.emit: {} records, {} piece offsets, {} / {} pieces'.format(len(rec_names), po.size, pc.size, pr.size))
        n = C.c_int64(0)
        rc = load().hhx_fasta_emit(self.h, os.fsencode(path), len(rec_names), ptr(blob), ptr(off), ptr(po), ptr(pc) if pc.size else None,
                                   ptr(pr) if pr.size else None, int(Ns), int(max_width), C.byref(n))
        check_served(rc, Fasta.Unsupported)
        return n.value

    def emit_segments(self, path, rec_names, piece_off, piece_ctg, piece_start, piece_len, piece_rev, max_width):
        """hhx_fasta_emit_segments: the records (rec_names: list of str; record r: pieces [piece_off[r], piece_off[r + 1])) as a FASTA file of
        max_width columns; piece k is bytes [piece_start[k], piece_start[k] + piece_len[k]) of contig piece_ctg[k], reversed and complemented where
        piece_rev[k], or piece_len[k] 'N' where piece_ctg[k] == -1; nothing between the pieces.  -> bytes written"""
        blob, off = names_blob(rec_names)
        po, pc = np.ascontiguousarray(piece_off, np.int64), np.ascontiguousarray(piece_ctg, np.int32)
        ps, pl = np.ascontiguousarray(piece_start, np.int64), np.ascontiguousarray(piece_len, np.int64)
        pr = np.ascontiguousarray(piece_rev, np.uint8)
        if po.size != len(rec_names) + 1 or not (pc.size == ps.size == pl.size == pr.size) or (po.size and pc.size != po[-1]):
            raise ValueError('Fasta.emit_segments: {} records, {} piece offsets, {} / {} / {} / {} pieces'.format(len(rec_names), po.size, pc.size, ps.size,
                                                                                                                  pl.size, pr.size))
        n = C.c_int64(0)
        some = pc.size > 0
        rc = load().hhx_fasta_emit_segments(self.h, os.fsencode(path), len(rec_names), ptr(blob), ptr(off), ptr(po), ptr(pc) if some else None,
                                            ptr(ps) if some else None, ptr(pl) if some else None, ptr(pr) if some else None, int(max_width), C.byref(n))
        check_served(rc, Fasta.Unsupported)
        return n.value


class Paf:
    """hhx_paf: the lines of one PAF file read on the device (parse_paf, HapHiC_refsort.py:81-134).  source: a path (str / os.PathLike) or the bytes
    of the file.  As with Gfa the library's handle holds the table on the host and nothing on the device, so the constructor copies the table —
    names() in first-seen order, query / target (name ids, int32), query_start, query_end, target_start, target_end, mapq (int64), plus (bool) per
    line that is not blank — and releases the handle before it returns, whatever happens: the object owns nothing and is no Handle; close() and
    `with` exist for callers that treat every reader alike.  tests/refsort_cases.py holds a host stand-in with the same interface.  Raises
    Unsupported where the library answers HHX_UNSUPPORTED (include/haphic_hip.h lists the cases); no handle was made then."""

    class Unsupported(RuntimeError):
        pass

    def __init__(self, source):
        h = C.c_void_p()
        if isinstance(source, (str, os.PathLike)):
            rc = load().hhx_paf_open(os.fsencode(source), C.byref(h))
        else:
            buf = np.frombuffer(source, np.uint8)
            rc = load().hhx_paf_open_bytes(ptr(buf) if buf.size else None, buf.size, C.byref(h))
        check_served(rc, Paf.Unsupported)
        try:
            n, nn, nb = C.c_int64(0), C.c_int64(0), C.c_int64(0)
            check(load().hhx_paf_counts(h, C.byref(n), C.byref(nn), C.byref(nb)))
            self.n_rec, self.n_names = n.value, nn.value
            self.name_off, self.name_bytes = np.zeros(self.n_names + 1, np.int64), np.zeros(max(nb.value, 1), np.uint8)
            self.query, self.target = np.zeros(self.n_rec, np.int32), np.zeros(self.n_rec, np.int32)
            self.query_start, self.query_end, self.target_start, self.target_end, self.mapq = (np.zeros(self.n_rec, np.int64) for _ in range(5))
            plus = np.zeros(self.n_rec, np.uint8)
            check(load().hhx_paf_table(h, ptr(self.name_off), ptr(self.name_bytes), ptr(self.query), ptr(self.target), ptr(self.query_start),
                                       ptr(self.query_end), ptr(self.target_start), ptr(self.target_end), ptr(self.mapq), ptr(plus)))
            self.name_bytes = self.name_bytes[:nb.value]
            self.plus = plus.astype(bool)
        finally:
            load().hhx_paf_close(h)

    def names(self):
        """fields 0 and 5 of all lines, each name once, in first-seen order (the text is ASCII: a byte >= 0x80 is refused)"""
        blob, off = self.name_bytes.tobytes().decode('ascii'), self.name_off.tolist()
        return [blob[off[k]:off[k + 1]] for k in range(self.n_names)]

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass


class LisUnsupported(RuntimeError):
    """hhx_lis_sums answered HHX_UNSUPPORTED: the caller takes the reference's function"""


def lis_sums(ptr_, value, weight):
    """hhx_lis_sums: (sums_f, sums_r), int64 per sequence — both find_lis sums (HapHiC_refsort.py:175-214) of the sequences
    [ptr_[s], ptr_[s + 1]) of value (int64 keys) and weight.  tests/refsort_cases.py holds a host engine with the same signature.  Raises
    LisUnsupported where the library answers HHX_UNSUPPORTED."""
    p, v, w = np.ascontiguousarray(ptr_, np.int64), np.ascontiguousarray(value, np.int64), np.ascontiguousarray(weight, np.int64)
    if p.ndim != 1 or p.size < 1 or v.shape != w.shape or v.ndim != 1 or int(p[-1]) != v.size:
        raise ValueError('lis_sums: {} offsets, {} values, {} weights'.format(p.shape, v.shape, w.shape))
    n = p.size - 1
    sf, sr = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64)
    rc = load().hhx_lis_sums(n, ptr(p), ptr(v) if v.size else None, ptr(w) if w.size else None, ptr(sf), ptr(sr))
    check_served(rc, LisUnsupported)
    return sf[:n], sr[:n]


class Gfa:
    """hhx_gfa: the S records of one GFA file read on the device (parse_gfa, HapHiC_cluster.py:150-185).  source: a path (str / os.PathLike) or the
    bytes of the file.  The library's handle holds the table on the host and nothing on the device, so the constructor copies the table —
    names() in file order, lengths and depths int64 — and releases the handle before it returns, whatever happens: the object owns nothing and is
    no Handle; close() and `with` exist for callers that treat every reader alike.  tests/assembly_cases.py holds a host stand-in with the same
    interface.  Raises Unsupported where the library answers HHX_UNSUPPORTED (include/haphic_hip.h lists the cases); no handle was made then."""

    class Unsupported(RuntimeError):
        pass

    def __init__(self, source):
        h = C.c_void_p()
        if isinstance(source, (str, os.PathLike)):
            rc = load().hhx_gfa_open(os.fsencode(source), C.byref(h))
        else:
            buf = np.frombuffer(source, np.uint8)
            rc = load().hhx_gfa_open_bytes(ptr(buf) if buf.size else None, buf.size, C.byref(h))
        check_served(rc, Gfa.Unsupported)
        try:
            n, nn = C.c_int64(0), C.c_int64(0)
            check(load().hhx_gfa_counts(h, C.byref(n), C.byref(nn)))
            self.n_rec = n.value
            self.name_off, self.name_bytes = np.zeros(self.n_rec + 1, np.int64), np.zeros(max(nn.value, 1), np.uint8)
            self.lengths, self.depths = np.zeros(self.n_rec, np.int64), np.zeros(self.n_rec, np.int64)
            check(load().hhx_gfa_table(h, ptr(self.name_off), ptr(self.name_bytes), ptr(self.lengths), ptr(self.depths)))
            self.name_bytes = self.name_bytes[:nn.value]
        finally:
            load().hhx_gfa_close(h)

    def names(self):
        """field 1 of every record in file order (the text is ASCII: a byte >= 0x80 is refused)"""
        blob, off = self.name_bytes.tobytes().decode('ascii'), self.name_off.tolist()
        return [blob[off[k]:off[k + 1]] for k in range(self.n_rec)]

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass


def allelic_nonmax(ki, kj, kcnt, n_ctg, gptr, gmem):
    """hhx_allelic_nonmax — the links between non-maximum matches :621-667: (mask uint8 [n_keys], counters int64 [3] = candidates, distinct group
    pairs, assignment problems), None when an `assert` of :652-659 would fail, NotImplemented when the library does not serve the call (an allele
    group of more than 8 contigs).  gptr / gmem: the groups in the reference's tuple order as contig ids."""
    ki, kj = np.ascontiguousarray(ki, np.int32), np.ascontiguousarray(kj, np.int32)
    kcnt = np.ascontiguousarray(kcnt, np.int64)
    gptr, gmem = np.ascontiguousarray(gptr, np.int64), np.ascontiguousarray(gmem, np.int32)
    if not (len(ki) == len(kj) == len(kcnt)) or len(gptr) < 1 or int(gptr[-1]) != len(gmem):
        raise ValueError('allelic_nonmax: ki, kj, kcnt of one length; gptr[-1] == len(gmem)')
    mask, counters, bad = np.zeros(len(ki), np.uint8), np.zeros(3, np.int64), C.c_int32(0)
    rc = load().hhx_allelic_nonmax(len(ki), ptr(ki), ptr(kj), ptr(kcnt), int(n_ctg), len(gptr) - 1, ptr(gptr), ptr(gmem), ptr(mask), ptr(counters), C.byref(bad))
    if not check_served(rc):
        return NotImplemented
    return None if bad.value else (mask, counters)


def lsap_small(cost):
    """hhx_lsap_small: col4row int32 [n, d] of scipy.optimize.linear_sum_assignment on every d x d matrix of cost [n, d, d] (int64, minimised), d <= 8"""
    cost = np.ascontiguousarray(cost, np.int64)
    if cost.ndim != 3 or cost.shape[1] != cost.shape[2]:
        raise ValueError('lsap_small: cost [n, d, d]')
    out = np.zeros(cost.shape[:2], np.int32)
    check(load().hhx_lsap_small(cost.shape[0], cost.shape[1], ptr(cost), ptr(out)))
    return out


def row_products(a, b):
    """products per row of a * b (int64 numpy)"""
    out = np.zeros(max(a.shape3[0], 1), np.int64)
    check(load().hhx_row_products(a.h, b.h, ptr(out)))
    return out[:a.shape3[0]]


def expand_links(links, r0, r1, inflation, pruning, fx_shift=52):
    """iteration 0 of mcl() for the rows [r0, r1) of the RAW link matrix `links` (the whole matrix: the right operand)"""
    out = C.c_void_p()
    f, z = C.c_int64(0), C.c_int64(0)
    check(load().hhx_expand_links(links.h, int(r0), int(r1), int(fx_shift), float(inflation), float(pruning), C.byref(out), C.byref(f), C.byref(z)))
    return DeviceCSR(out), f.value, z.value


def mcl(pre_expanded, expansion, inflation, max_iter, pruning, want_stats=False, normalized=False, links=False):
    """normalized=False: the reference seam (matrix already pre-expanded); True: start from the
    L1-normalised link matrix, pre-expansion fused into iteration 0 (hhx_mcl_normalized); links=True: start
    from the raw link matrix of dict_to_matrix (hhx_mcl_links: normalisation fused too)."""
    out = C.c_void_p()
    n_iter, conv = C.c_int(0), C.c_int(0)
    stats = np.zeros((max(int(max_iter), 1), 4), np.int64)
    fn = load().hhx_mcl_links if links else (load().hhx_mcl_normalized if normalized else load().hhx_mcl)
    check(fn(pre_expanded.h, int(expansion), float(inflation), int(max_iter), float(pruning),
                         C.byref(out), C.byref(n_iter), C.byref(conv), ptr(stats)))
    res = (DeviceCSR(out), n_iter.value, bool(conv.value))
    return res + (stats[:n_iter.value],) if want_stats else res


def interpret(m):
    r, _, z = m.shape3
    att = np.empty(max(r, 1), np.int32)
    att_ptr = np.empty(r + 1, np.int32)
    members = np.empty(max(z, 1), np.int32)
    na = C.c_int32(0)
    check(load().hhx_interpret(m.h, ptr(att), ptr(att_ptr), ptr(members), C.byref(na)))
    na = na.value
    return att[:na], att_ptr[:na + 1], members[:att_ptr[na]]


def dict_to_matrix(frag_i, frag_j, value, n_frag, in_set, n_rest, add_self_loops=True, on_device=False, n_keys=None):
    """frag_i/frag_j/value: numpy arrays (on_device=False) or raw device pointers (ints, on_device=True)."""
    in_set = np.ascontiguousarray(in_set, np.uint8)
    frag_index = np.empty(max(n_frag, 1), np.int32)
    n_linked = C.c_int32(0)
    if on_device:
        a, b, v = C.c_void_p(frag_i), C.c_void_p(frag_j), C.c_void_p(value)
        nk = int(n_keys)
    else:
        fi = np.ascontiguousarray(frag_i, np.int32)
        fj = np.ascontiguousarray(frag_j, np.int32)
        fv = np.ascontiguousarray(value, np.float64)
        a, b, v = ptr(fi), ptr(fj), ptr(fv)
        nk = fi.size
    out = new_handle('hhx_dict_to_matrix', nk, a, b, v, int(on_device), int(n_frag), ptr(in_set), int(n_rest), int(add_self_loops), ptr(frag_index),
                     C.byref(n_linked))
    return DeviceCSR(out), frag_index[:n_frag], n_linked.value


def rank_sums(m, topN):
    """filter_fragments' rank-sum statistic of every row of the (self-loop free) link matrix"""
    out = np.zeros(max(m.shape3[0], 1), np.int64)
    check(load().hhx_rank_sums(m.h, int(topN), ptr(out)))
    return out[:m.shape3[0]]


def count_re_sites(seq, seg_off, seg_len, sites):
    """seq: bytes-like / uint8 array; sites: list of bytes patterns (already N-expanded).  Returns int64 counts."""
    buf = np.frombuffer(seq, np.uint8) if not isinstance(seq, np.ndarray) else np.ascontiguousarray(seq, np.uint8)
    off = np.ascontiguousarray(seg_off, np.int64)
    ln = np.ascontiguousarray(seg_len, np.int64)
    pats = np.frombuffer(b''.join(sites), np.uint8) if sites else np.zeros(1, np.uint8)
    plen = np.array([len(x) for x in sites], np.int32) if sites else np.zeros(1, np.int32)
    out = np.zeros(max(off.size, 1), np.int64)
    check(load().hhx_count_re_sites(ptr(buf) if buf.size else None, buf.size, off.size, ptr(off), ptr(ln), len(sites), ptr(pats),
                                    ptr(plen), ptr(out)))
    return out[:off.size]


class BamReader(Handle):
    """hhx_bam: BGZF / BAM container -> batches of device id / position arrays (f4)."""
    _release = 'hhx_bam_close'

    def __init__(self, path, threads=0):
        self.h = new_handle('hhx_bam_open', os.fsencode(path), int(threads))
        n_ref, text, tlen = C.c_int32(0), C.c_char_p(), C.c_int64(0)
        names, offs = C.c_void_p(), C.c_void_p()
        try:
            check(load().hhx_bam_header(self.h, C.byref(n_ref), C.byref(text), C.byref(tlen), C.byref(names), C.byref(offs)))
        except RuntimeError:
            self.close()                # not left to the finaliser: the file and the reader threads go now
            raise
        self.header_text = C.string_at(text, tlen.value).decode('utf-8', 'replace') if tlen.value else ''
        off = np.ctypeslib.as_array(C.cast(offs, C.POINTER(C.c_int64)), (n_ref.value + 1,)).copy() if n_ref.value else np.zeros(1, np.int64)
        blob = C.string_at(names, int(off[-1])) if n_ref.value and off[-1] else b''
        self.ref_names = [blob[off[k]:off[k + 1]].decode() for k in range(n_ref.value)]
        self._map = None

    def set_contigs(self, ctg_ids):
        """ctg_ids: name -> contig id of the FASTA; BAM references outside it map to -1 (`ref not in fa_dict`)"""
        self._map = np.fromiter((ctg_ids.get(n, -1) for n in self.ref_names), np.int32, len(self.ref_names))
        if not len(self._map):
            self._map = np.zeros(0, np.int32)

    def next_batch(self, need_flags, drop_same_ref, max_inflated_bytes=256 << 20):
        """-> (n_records, [id1, pos1, id2, pos2] device pointers); n_records == 0 at the end of the file"""
        n = C.c_int64(0)
        p = [C.c_void_p() for _ in range(4)]
        check(load().hhx_bam_next(self.h, int(need_flags), int(drop_same_ref), len(self.ref_names), ptr(self._map) if len(self._map) else None,
                                  int(max_inflated_bytes), C.byref(n), *[C.byref(x) for x in p]))
        self.last_n = n.value
        return n.value, [x.value for x in p]

    def fetch(self):
        """host copies (id1, pos1, id2, pos2) of the last batch"""
        out = [np.empty(self.last_n, np.int32) for _ in range(4)]
        check(load().hhx_bam_fetch(self.h, *[ptr(a) for a in out]))
        return out


class ContactMap(Handle):
    """hhx_contact_map: the dense scaffold-bin contact matrix of `haphic plot` (f4).  Tables as include/haphic_hip.h lists them."""
    _release = 'hhx_contact_map_destroy'

    def __init__(self, in_set, aln_ptr, list_ptr, seg_lo, seg_hi, seg_bin, bin_size, n_total_bins):
        self.in_set = np.ascontiguousarray(in_set, np.uint8)
        self.aln_ptr = np.ascontiguousarray(aln_ptr, np.int64)
        self.list_ptr = np.ascontiguousarray(list_ptr, np.int32)
        self.seg = [np.ascontiguousarray(a, np.int32) for a in (seg_lo, seg_hi, seg_bin)]
        self.n_bins = int(n_total_bins)
        self.h = new_handle('hhx_contact_map_create', len(self.in_set), ptr(self.in_set), ptr(self.aln_ptr), ptr(self.list_ptr), len(self.seg[0]),
                            ptr(self.seg[0]), ptr(self.seg[1]), ptr(self.seg[2]), int(bin_size), self.n_bins)

    def _push(self, n, p, on_device, pos_offset):
        bad = C.c_int64(-1)
        check(load().hhx_contact_map_push(self.h, int(n), p[0], p[1], p[2], p[3], int(on_device), int(pos_offset), C.byref(bad)))
        return bad.value

    def push(self, id1, pos1, id2, pos2, pos_offset=0):
        """host int32 arrays; -> -1, or 2 * k + side of the first pair whose position is outside the AGP"""
        arrs = [np.ascontiguousarray(a, np.int32) for a in (id1, pos1, id2, pos2)]
        return self._push(len(arrs[0]), [ptr(a) for a in arrs], False, pos_offset)

    def push_device(self, n, id1, pos1, id2, pos2, pos_offset=0):
        return self._push(n, [C.c_void_p(x) for x in (id1, pos1, id2, pos2)], True, pos_offset)

    def fetch(self):
        out = np.empty((self.n_bins, self.n_bins), np.int64)
        check(load().hhx_contact_map_fetch(self.h, ptr(out)))
        return out


class PlotNorm(Handle):
    """hhx_plotnorm: the scaffold-bin matrix of `haphic plot` in HBM as int32 counts, for the Knight-Ruiz balancing, the scaled matrix and the
    off-diagonal median of HapHiC_plot.py normalize_matrix :407-504 (include/haphic_hip.h).  .max / .min / .symmetric describe the upload."""
    _release = 'hhx_plotnorm_destroy'

    def __init__(self, matrix):
        matrix = np.ascontiguousarray(matrix, np.int64)
        assert matrix.ndim == 2 and matrix.shape[0] == matrix.shape[1]
        self.n = matrix.shape[0]
        self.h = C.c_void_p()
        mx, mn, sym = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        check(load().hhx_plotnorm_create(ptr(matrix), self.n, C.byref(self.h), C.byref(mx), C.byref(mn), C.byref(sym)))
        self.max, self.min, self.symmetric = mx.value, mn.value, bool(sym.value)
        self.n_blocks = 0

    def set_blocks(self, lo, hi):
        lo, hi = np.ascontiguousarray(lo, np.int32), np.ascontiguousarray(hi, np.int32)
        check(load().hhx_plotnorm_set_blocks(self.h, len(lo), ptr(lo), ptr(hi)))
        self.n_blocks = len(lo)

    def balance(self):
        """-> (outer steps, mat-vec counts, status) per block, the whole matrix last; status 1: a cap of bnewt was reached"""
        outer, mvp, status = np.zeros(self.n_blocks + 1, np.int32), np.zeros(self.n_blocks + 1, np.int64), np.zeros(self.n_blocks + 1, np.int32)
        check(load().hhx_plotnorm_balance(self.h, ptr(outer), ptr(mvp), ptr(status)))
        return outer, mvp, status

    def x(self):
        """-> (x of the whole matrix, the blocks' x at their bins)"""
        x_all, x_blk = np.empty(self.n), np.empty(self.n)
        check(load().hhx_plotnorm_fetch_x(self.h, ptr(x_all), ptr(x_blk)))
        return x_all, x_blk

    def apply(self):
        out = np.empty((self.n, self.n), np.float64)
        check(load().hhx_plotnorm_apply(self.h, ptr(out)))
        return out

    def middle(self, kr):
        """-> (count, lo, hi): the two middle off-diagonal block cells, float64 (kr) or int64 counts"""
        count, lo, hi = C.c_int64(0), C.c_uint64(0), C.c_uint64(0)
        check(load().hhx_plotnorm_median(self.h, int(bool(kr)), C.byref(count), C.byref(lo), C.byref(hi)))
        pair = np.array([lo.value, hi.value], np.uint64)
        return count.value, pair.view(np.float64) if kr else pair.astype(np.int64)

    def matvec(self, lo, hi, v):
        v = np.ascontiguousarray(v, np.float64)
        assert len(v) == hi - lo
        out = np.empty(hi - lo)
        check(load().hhx_plotnorm_matvec(self.h, int(lo), int(hi), ptr(v), ptr(out)))
        return out


def select_middle(values):
    """the two middle values of a non-negative float64 array (radix select over the bit patterns on the device); None when it is empty"""
    values = np.ascontiguousarray(values, np.float64)
    lo, hi = C.c_uint64(0), C.c_uint64(0)
    check(load().hhx_select_middle_u64(ptr(values), len(values), C.byref(lo), C.byref(hi)))
    return np.array([lo.value, hi.value], np.uint64).view(np.float64) if len(values) else None


class PairsParser(Handle):
    """hhx_pairs_parser: .pairs text chunks -> device id / position arrays (+ the alignments.bed bytes)."""
    _release = 'hhx_pairs_parser_destroy'

    def __init__(self, names):
        blob, off = names_blob(names)
        self.h = new_handle('hhx_pairs_parser_create', len(off) - 1, ptr(blob), ptr(off))
        self.n_lines = self.bed_bytes = 0
        self.wide = False

    def set_wide(self, on=True):
        """positions as int64 from the next parse on (contigs of 2^31 bp and more)"""
        check(load().hhx_pairs_parser_set_wide(self.h, int(on)))
        self.wide = bool(on)

    def parse(self, text, want_bed=False, device_ptr=None, n_bytes=None, host_ptr=None):
        """text: bytes-like holding whole lines (or device_ptr / host_ptr + n_bytes); raises IndexError / ValueError like
        the reference's cols[k] / int() do"""
        nl, nb = C.c_int64(0), C.c_int64(0)
        if host_ptr is not None:
            rc = load().hhx_pairs_parse(self.h, C.c_void_p(host_ptr), int(n_bytes), 0, int(want_bed), C.byref(nl), C.byref(nb))
        elif device_ptr is None:
            buf = np.frombuffer(text, np.uint8)
            rc = load().hhx_pairs_parse(self.h, ptr(buf) if buf.size else None, buf.size, 0, int(want_bed), C.byref(nl), C.byref(nb))
        else:
            rc = load().hhx_pairs_parse(self.h, C.c_void_p(device_ptr), int(n_bytes), 1, int(want_bed), C.byref(nl), C.byref(nb))
        check_py(rc)
        self.n_lines, self.bed_bytes = nl.value, nb.value
        return self.n_lines

    def device_arrays(self):
        p = [C.c_void_p() for _ in range(5)]
        check(load().hhx_pairs_parser_arrays(self.h, *[C.byref(x) for x in p]))
        return [x.value for x in p]

    def fetch(self, want_bed=False):
        out = [np.empty(self.n_lines, np.int64 if self.wide and k in (1, 3) else np.int32) for k in range(4)]
        bed = np.empty(self.bed_bytes if want_bed else 0, np.uint8)
        fn = load().hhx_pairs_parser_fetch64 if self.wide else load().hhx_pairs_parser_fetch
        check(fn(self.h, *[ptr(a) for a in out], ptr(bed) if bed.size else None))
        return out + [bed.tobytes()]

    def format_pairs(self, n, id1_ptr, pos1_ptr, id2_ptr, pos2_ptr, first_read=0, text_ptr=None, capacity=0):
        """measurement only: device id / position arrays -> .pairs text on the device (hhx_pairs_format); returns the byte count
        (text_ptr None: just the size)"""
        nb = C.c_int64(0)
        check(load().hhx_pairs_format(self.h, int(n), C.c_void_p(id1_ptr), C.c_void_p(pos1_ptr), C.c_void_p(id2_ptr), C.c_void_p(pos2_ptr), int(first_read),
                                      C.c_void_p(text_ptr) if text_ptr else None, int(capacity), C.byref(nb)))
        return nb.value

    def set_bed_sink(self, sink):
        """from the next parse(want_bed=True) on the BED records are formatted into the ByteSink's ring in HBM and queued for the file-writer
        thread (None: back to the parser's own buffer)"""
        check(load().hhx_pairs_parser_set_bed_sink(self.h, sink.h if sink is not None else None))

    def bed_host(self):
        """the alignments.bed bytes of the last parse as a uint8 VIEW of pinned memory owned by the parser (valid until the
        second following call)"""
        host, n = C.c_void_p(), C.c_int64(0)
        check(load().hhx_pairs_parser_bed_host(self.h, C.byref(host), C.byref(n)))
        if not n.value:
            return np.zeros(0, np.uint8)
        return np.ctypeslib.as_array(C.cast(host, C.POINTER(C.c_uint8)), (n.value,))

    def fetch_bed(self):
        """the alignments.bed bytes of the last parse (uint8 array)"""
        bed = np.empty(self.bed_bytes, np.uint8)
        if self.bed_bytes:
            check(load().hhx_pairs_parser_fetch(self.h, None, None, None, None, ptr(bed)))
        return bed


class Ingest(Handle):
    """hhx_ingest handle: push batches of (id1, pos1, id2, pos2), then finalize/fetch."""
    _release = 'hhx_ingest_destroy'

    def __init__(self, table, flank, bins=False, skip_intra=False, expected_keys=0):
        self._keep = table      # keeps the numpy arrays alive during create
        cfg = IngestConfig()
        cfg.n_ctg, cfg.n_frag = table.n_ctg, table.n_frag
        cfg.ctg_rank = table.ctg_rank.ctypes.data_as(c_i32p)
        cfg.ctg_len = table.ctg_len.ctypes.data_as(c_i64p)
        cfg.ctg_frag0 = table.ctg_frag0.ctypes.data_as(c_i32p)
        cfg.ctg_split = table.ctg_split.ctypes.data_as(c_u8p)
        cfg.frag_rank = table.frag_rank.ctypes.data_as(c_i32p)
        cfg.frag_len = table.frag_len.ctypes.data_as(c_i64p)
        cfg.frag_nx = table.frag_nx.ctypes.data_as(c_u8p)
        cfg.bin_size, cfg.flank = int(table.bin_size), int(flank)
        cfg.bins, cfg.skip_intra = int(bool(bins)), int(bool(skip_intra))
        cfg.expected_keys = int(expected_keys)
        self.n_frag = table.n_frag
        self.h = new_handle('hhx_ingest_create', C.byref(cfg))
        self.n_full = self.n_flank = None

    def push(self, id1, pos1, id2, pos2, wide=None):
        """host arrays.  wide=True: 64-bit positions through hhx_ingest_push64 (contigs of 2^31 bp and more, :116-147).  wide=None:
        decided by the VALUES, not the dtype — default-int64 numpy arrays whose positions fit 32 bits take the packed 32-bit path
        (half the host-to-device bytes, four pairs per lane in the map kernel)."""
        pos = [np.asarray(pos1), np.asarray(pos2)]
        i32max = np.iinfo(np.int32).max
        # by VALUE, whatever the dtype (a uint32 array can hold 2^31 and more; an int64 array usually does not)
        beyond = any(a.dtype != np.int32 and a.size and int(a.max()) > i32max for a in pos)
        if wide is None:
            wide = beyond
        elif not wide and beyond:
            raise ValueError('Ingest.push(wide=False): a position exceeds the int32 range; pass wide=True (hhx_ingest_push64)')
        if any(a.dtype != np.int32 and a.dtype.kind == 'i' and a.size and int(a.min()) < -i32max - 1 for a in pos):
            raise ValueError('Ingest.push: a position below the int32 range')
        if wide:
            ids = [np.ascontiguousarray(a, np.int32) for a in (id1, id2)]
            pos = [np.ascontiguousarray(a, np.int64) for a in (pos1, pos2)]
            check(load().hhx_ingest_push64(self.h, ids[0].size, ptr(ids[0]), ptr(pos[0]), ptr(ids[1]), ptr(pos[1]), 0))
            return
        arrs = [np.ascontiguousarray(a, np.int32) for a in (id1, pos1, id2, pos2)]
        check(load().hhx_ingest_push(self.h, arrs[0].size, *[ptr(a) for a in arrs], 0))

    def push_device(self, n_pairs, id1_ptr, pos1_ptr, id2_ptr, pos2_ptr, wide=False):
        """device arrays (int32 ids; positions int32, or int64 with wide=True)"""
        fn = load().hhx_ingest_push64 if wide else load().hhx_ingest_push
        check(fn(self.h, int(n_pairs), C.c_void_p(id1_ptr), C.c_void_p(pos1_ptr), C.c_void_p(id2_ptr), C.c_void_p(pos2_ptr), 1))

    def finalize(self):
        a, b = C.c_int64(0), C.c_int64(0)
        check(load().hhx_ingest_finalize(self.h, C.byref(a), C.byref(b)))
        self.n_full, self.n_flank = a.value, b.value
        return self.n_full, self.n_flank

    _FETCH = ('full_i', 'full_j', 'full_cnt', 'ht_cnt', 'flank_i', 'flank_j', 'flank_cnt', 'frag_links')

    def fetch(self, want=None):
        """host copies in dict insertion order (hhx_ingest_fetch); want: the subset of _FETCH to copy (default: all)"""
        if self.n_full is None:
            self.finalize()
        nf, nk = self.n_full, self.n_flank
        shape = dict(full_i=(nf, np.int32), full_j=(nf, np.int32), full_cnt=(nf, np.int64), ht_cnt=((nf, 4), np.int64),
                     flank_i=(nk, np.int32), flank_j=(nk, np.int32), flank_cnt=(nk, np.int64), frag_links=(self.n_frag, np.int64))
        want = self._FETCH if want is None else tuple(want)
        out = {k: np.empty(*shape[k]) for k in want}
        check(load().hhx_ingest_fetch(self.h, *[ptr(out[k]) if k in out else None for k in self._FETCH]))
        return out

    def fetch_flank_values(self):
        """the float64 values of the flank table in dict order (counts, or the weights hhx_link_weights left there)"""
        out = np.empty(self.n_flank, np.float64)
        check(load().hhx_ingest_fetch_flank_values(self.h, ptr(out)))
        return out

    def weigh_flank(self, mode, per_frag=None, tag=None, param=0.0):
        """hhx_link_weights on the device-resident flank table (normalize_by_nlinks :718-724 and friends): the weights never
        leave HBM on their way into link_matrix(weighted=True)"""
        pi, pj, pv = self.flank_device()
        return link_weights(None, None, None, mode, self.n_frag, per_frag=per_frag, tag=tag, param=param,
                            device_ptrs=(self.n_flank, pi, pj, pv))

    def flank_device(self):
        a, b, v = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(load().hhx_ingest_flank_device(self.h, C.byref(a), C.byref(b), C.byref(v)))
        return a.value or 0, b.value or 0, v.value or 0

    def flank_count_device(self):
        c = C.c_void_p()
        check(load().hhx_ingest_flank_count_device(self.h, C.byref(c)))
        return c.value or 0

    def keep_pairs(self, on=True):
        """also keep the oriented coordinates of every counted pair (CLM / coordinate side products)"""
        check(load().hhx_ingest_keep_pairs(self.h, int(on)))

    def fetch_pairs(self, max_read_pairs, full_cnt):
        """(clm_ptr, clm, crd_ptr, crd) in dict insertion order; clm_ptr counts READ PAIRS (x 4 values each)"""
        nf = len(full_cnt)
        total = int(np.sum(full_cnt))
        capped = int(np.minimum(full_cnt, max_read_pairs).sum()) if max_read_pairs > 0 else 0
        clm_ptr = np.zeros(nf + 1, np.int64)
        crd_ptr = np.zeros(nf + 1, np.int64)
        clm = np.zeros(max(4 * total, 1), np.int64)
        crd = np.zeros(max(2 * capped, 1), np.int64)
        check(load().hhx_ingest_fetch_pairs(self.h, int(max_read_pairs), ptr(clm_ptr), ptr(clm), ptr(crd_ptr), ptr(crd)))
        return clm_ptr, clm[:4 * total], crd_ptr, crd[:2 * capped]

    def fetch_ht_order(self):
        """[n_full, 4] stream positions of the first pair per head/tail quadrant (INT64_MAX: none): HT_link_dict's order"""
        first = np.full((max(self.n_full, 1), 4), np.iinfo(np.int64).max, np.int64)
        check(load().hhx_ingest_fetch_ht_order(self.h, ptr(first)))
        return first[:self.n_full]

    def fetch_ht_items(self):
        """HT_link_dict in insertion order: (name_i, name_j, count) with name ids 2 * contig + (1 for '_T'); ordered on the device"""
        n = C.c_int64(0)
        check(load().hhx_ingest_fetch_ht_items(self.h, C.byref(n), None, None, None))
        ni, nj, cnt = np.empty(n.value, np.int32), np.empty(n.value, np.int32), np.empty(n.value, np.int64)
        if n.value:
            check(load().hhx_ingest_fetch_ht_items(self.h, C.byref(n), ptr(ni), ptr(nj), ptr(cnt)))
        return ni, nj, cnt

    def n_ht_items(self):
        n = C.c_int64(0)
        check(load().hhx_ingest_fetch_ht_items(self.h, C.byref(n), None, None, None))
        return n.value

    UNSUPPORTED = HHX_UNSUPPORTED

    def concordance_counts(self, max_read_pairs, nwindows, min_read_pairs=0):
        """cal_concordance_ratio :419-428 as integers (hhx_ingest_concordance): (m, diag, anti) int32 arrays in full_link_dict order —
        m = min(count, max_read_pairs), the modal counts of the diagonal / anti-diagonal windows of the key's first m read pairs; the
        ratio is max(diag / m, anti / m).  Keys with m < min(min_read_pairs, max_read_pairs) get 0 / 0.  None: the library does not
        serve this call (max_read_pairs beyond its cap, a contig shorter than nwindows)."""
        if self.n_full is None:
            self.finalize()
        m, diag, anti = (np.zeros(self.n_full, np.int32) for _ in range(3))
        rc = load().hhx_ingest_concordance(self.h, int(max_read_pairs), int(min_read_pairs), int(nwindows), ptr(m), ptr(diag), ptr(anti))
        return (m, diag, anti) if check_served(rc) else None

    def drop_links(self, full_drop, in_set):
        """update_link_dicts :488-509 for a whole verdict (hhx_ingest_drop_links): full_drop — one flag per full_link_dict key, in_set — one per
        fragment (filtered_frags).  Returns (n_full, n_flank, flank_dropped, remaining) — the sizes afterwards, which flank keys left (dict order
        before the call) and which fragments of in_set still have a flank key inside in_set (:680-683; self.first_row orders them as that loop
        meets them) — or None when the library does not serve the call.  The handle's tables are the smaller dicts from then on."""
        if self.n_full is None:
            self.finalize()
        full_drop = np.ascontiguousarray(full_drop, np.uint8)
        in_set = np.ascontiguousarray(in_set, np.uint8)
        if full_drop.shape != (self.n_full,) or in_set.shape != (self.n_frag,):
            raise ValueError('Ingest.drop_links: one flag per full key ({}) and per fragment ({})'.format(self.n_full, self.n_frag))
        a, b = C.c_int64(0), C.c_int64(0)
        gone = np.zeros(self.n_flank, np.uint8)
        remaining = np.zeros(self.n_frag, np.uint8)
        first_row = np.full(self.n_frag, -1, np.int64)
        rc = load().hhx_ingest_drop_links(self.h, ptr(full_drop), ptr(in_set), C.byref(a), C.byref(b), ptr(gone), ptr(remaining), ptr(first_row))
        if not check_served(rc):
            return None
        self.n_full, self.n_flank = a.value, b.value
        self.first_row = first_row
        return self.n_full, self.n_flank, gone, remaining

    def group_stats(self, group, n_groups, group_re, ctg_re, sum_mode=0):
        """group_stats (above) on the contig-pair table of this handle as it is now (hhx_ingest_group_stats): the keys of full_link_dict never
        leave the device.  group is [n_sets, n_ctg] over the contig ids of the handle.  None: not served."""
        if self.n_full is None:
            self.finalize()
        grp, ng, gre, cre, out = _group_stats_args(group, n_groups, group_re, ctg_re)
        rc = load().hhx_ingest_group_stats(self.h, grp.shape[0], ptr(grp), ptr(ng), ptr(gre), ptr(cre), int(sum_mode), *[ptr(a) for a in out])
        return out if check_served(rc) else None

    def keep_frag_pairs(self, on=True):
        check(load().hhx_ingest_keep_frag_pairs(self.h, int(on)))

    def fetch_frag_pairs(self):
        """every distinct oriented fragment pair of the stream (ctg_pair_to_frag :1731): (frag_i, frag_j) arrays"""
        n = C.c_int64(0)
        check(load().hhx_ingest_fetch_frag_pairs(self.h, C.byref(n), None, None))
        fi, fj = np.empty(n.value, np.int32), np.empty(n.value, np.int32)
        if n.value:
            check(load().hhx_ingest_fetch_frag_pairs(self.h, C.byref(n), ptr(fi), ptr(fj)))
        return fi, fj

    def set_ordinal_base(self, base):
        """global stream ordinal of this handle's first pair (multi-GPU chunk offset); before the first push"""
        check(load().hhx_ingest_set_ordinal_base(self.h, int(base)))

    def link_matrix(self, in_set, n_rest=-1, add_self_loops=True, weighted=False):
        """dict_to_matrix fused onto the device-resident flank table: (DeviceCSR, frag_index, n_linked).  weighted: the values
        are the float64 weights of weigh_flank (hhx_dict_to_matrix over the ordered device arrays) instead of the counts."""
        if self.n_full is None:
            self.finalize()
        in_set = np.ascontiguousarray(in_set, np.uint8)
        if weighted:
            pi, pj, pv = self.flank_device()
            return dict_to_matrix(pi, pj, pv, self.n_frag, in_set, n_rest, add_self_loops=add_self_loops, on_device=True,
                                  n_keys=self.n_flank)
        frag_index = np.empty(max(self.n_frag, 1), np.int32)
        n_linked = C.c_int32(0)
        out = new_handle('hhx_ingest_link_matrix', self.h, ptr(in_set), int(n_rest), int(add_self_loops), ptr(frag_index), C.byref(n_linked))
        return DeviceCSR(out), frag_index[:self.n_frag], n_linked.value

    def write_clm(self, path, ctg_names):
        """paired_links.clm (output_clm :376-392) from the kept read pairs: grouped, sorted and formatted on the device.
        Returns (lines, bytes) written."""
        blob, off = names_blob(ctg_names)
        n_lines, n_bytes = C.c_int64(0), C.c_int64(0)
        check(load().hhx_ingest_write_clm(self.h, os.fsencode(path), ptr(blob), ptr(off), C.byref(n_lines), C.byref(n_bytes)))
        return n_lines.value, n_bytes.value

    def write_clm_async(self, path, ctg_names, drop_pairs=False):
        """write_clm on the library's file-writer thread (hhx_ingest_write_clm_async): checked and opened here, complete after
        files_join(); drop_pairs: the kept read pairs leave HBM when the file is done"""
        blob, off = names_blob(ctg_names)
        _register_join()
        check(load().hhx_ingest_write_clm_async(self.h, os.fsencode(path), ptr(blob), ptr(off), int(bool(drop_pairs))))

    PICKLE_KINDS = {'full': 0, 'HT': 1, 'flank': 2}

    def write_link_pickle_async(self, kind, path, names):
        """full_links.pkl / HT_links.pkl (output_pickle :710-715) of this handle's table on the file-writer thread: the items are
        fetched (HT: ordered on the device) and encoded there; complete after files_join()"""
        blob, off = names_blob(names)
        _register_join()
        check(load().hhx_ingest_write_link_pickle_async(self.h, self.PICKLE_KINDS[kind], os.fsencode(path), len(names), ptr(blob), ptr(off)))

    def table_device(self, which=0):
        """aggregated table (unordered): (n_rows, key_ptr, ord_full_ptr, ord_flank_ptr, ht_ptr, flank_ptr)"""
        if self.n_full is None:
            self.finalize()
        n = C.c_int64(0)
        p = [C.c_void_p() for _ in range(5)]
        check(load().hhx_ingest_table_device(self.h, int(which), C.byref(n), *[C.byref(x) for x in p]))
        return (n.value,) + tuple(x.value or 0 for x in p)

    def push_table(self, which, n_rows, key_ptr, ord_full_ptr, ord_flank_ptr, ht_ptr, flank_ptr):
        check(load().hhx_ingest_push_table(self.h, int(which), int(n_rows), C.c_void_p(key_ptr), C.c_void_p(ord_full_ptr),
                                           C.c_void_p(ord_flank_ptr), C.c_void_p(ht_ptr), C.c_void_p(flank_ptr)))


class CorrectTable(Handle):
    """hhx_correct: coverage bins and (lo, hi) position lists of the intra-contig read pairs (pass one of --correct_nrounds), the
    break-point detection and the per-pair half of the breaking on them.  Segments = the contigs of the FASTA after finalize(), the
    children of the broken contigs after break_()."""
    _release = 'hhx_correct_destroy'

    def __init__(self, ctg_len, resolution):
        lens = np.ascontiguousarray(ctg_len, np.int64)
        self.resolution = int(resolution)
        self.h = new_handle('hhx_correct_create', len(lens), ptr(lens), self.resolution)

    def push(self, id1, pos1, id2, pos2):
        arrs = [np.ascontiguousarray(a, np.int32) for a in (id1, pos1, id2, pos2)]
        check(load().hhx_correct_push(self.h, arrs[0].size, *[ptr(a) for a in arrs], 0))

    def push_device(self, n, id1_ptr, pos1_ptr, id2_ptr, pos2_ptr):
        check(load().hhx_correct_push(self.h, int(n), C.c_void_p(id1_ptr), C.c_void_p(pos1_ptr), C.c_void_p(id2_ptr), C.c_void_p(pos2_ptr), 1))

    def finalize(self):
        n = C.c_int64(0)
        check(load().hhx_correct_finalize(self.h, C.byref(n)))
        return n.value

    def export_shape(self):
        """(resolution, bins, kept records) of a table that is not finalized"""
        r, b, p = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        check(load().hhx_correct_export(self.h, C.byref(r), C.byref(b), C.byref(p), None, 0, 0, None, None, 0))
        return r.value, b.value, p.value

    def export_diff(self):
        """host copy of the coverage difference array of a table that is not finalized"""
        diff = np.empty(self.export_shape()[1], np.int32)
        check(load().hhx_correct_export(self.h, None, None, None, ptr(diff) if diff.size else None, 0, 0, None, None, 0))
        return diff

    def export_pairs(self, first, count):
        """-> (pair_ctg int32 [count], pair_lo_hi int32 [2 count]): host copies of the kept records [first, first + count) in push order"""
        ctg, lo_hi = np.empty(count, np.int32), np.empty(2 * count, np.int32)
        if count:
            check(load().hhx_correct_export(self.h, None, None, None, None, int(first), int(count), ptr(ctg), ptr(lo_hi), 0))
        return ctg, lo_hi

    def export(self):
        """-> (resolution, cov_diff, pair_ctg, pair_lo_hi) of the whole table; absorb(*other.export()) adds them to another table"""
        res, _bins, n = self.export_shape()
        return (res, self.export_diff()) + self.export_pairs(0, n)

    def export_device(self, diff_ptr, first, count, ctg_ptr, lo_hi_ptr):
        """the same into device arrays (a null pointer: that part is left out)"""
        check(load().hhx_correct_export(self.h, None, None, None, C.c_void_p(diff_ptr), int(first), int(count), C.c_void_p(ctg_ptr),
                                        C.c_void_p(lo_hi_ptr), 1))

    def absorb(self, resolution, cov_diff, pair_ctg, pair_lo_hi):
        """add a piece of a partial table (host arrays) to this one, its records behind those kept so far.  cov_diff None: records alone (the
        difference array came with an earlier piece)"""
        n_bins = self.export_shape()[1] if cov_diff is None else len(cov_diff)
        diff = None if cov_diff is None else np.ascontiguousarray(cov_diff, np.int32)
        ctg, lo_hi = (np.ascontiguousarray(a, np.int32) for a in (pair_ctg, pair_lo_hi))
        if lo_hi.size != 2 * ctg.size:
            raise ValueError('CorrectTable.absorb: {} contig ids, {} positions'.format(ctg.size, lo_hi.size))
        check(load().hhx_correct_absorb(self.h, int(resolution), n_bins, ptr(diff) if diff is not None and diff.size else None, ctg.size,
                                        ptr(ctg) if ctg.size else None, ptr(lo_hi) if ctg.size else None, 0))

    def absorb_device(self, resolution, n_bins, diff_ptr, n_pairs, ctg_ptr, lo_hi_ptr):
        check(load().hhx_correct_absorb(self.h, int(resolution), int(n_bins), C.c_void_p(diff_ptr), int(n_pairs), C.c_void_p(ctg_ptr),
                                        C.c_void_p(lo_hi_ptr), 1))

    def shape(self):
        """(segments, bins of the flat coverage array, pairs)"""
        s, b, p = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        check(load().hhx_correct_shape(self.h, C.byref(s), C.byref(b), C.byref(p)))
        return s.value, b.value, p.value

    def segments(self):
        """(bin_off, n_bins, length, pair_off[n_seg + 1]) of the table"""
        n = self.shape()[0]
        out = np.empty(n, np.int64), np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n + 1, np.int64)
        check(load().hhx_correct_fetch_segments(self.h, *[ptr(a) for a in out]))
        return out

    def coverage(self):
        """the flat coverage array; segment s = [bin_off[s], bin_off[s] + n_bins[s])"""
        out = np.empty(self.shape()[1], np.int32)
        check(load().hhx_correct_fetch_coverage(self.h, ptr(out)))
        return out

    def pairs(self):
        """lo, hi interleaved, int32 [2 * n_pairs], segment order (segment s = items [2 * pair_off[s], 2 * pair_off[s + 1]))"""
        out = np.empty(2 * self.shape()[2], np.int32)
        check(load().hhx_correct_fetch_pairs(self.h, ptr(out)))
        return out

    def detect(self, median_cov_ratio, region_len_ratio, min_region_cutoff):
        """-> (n_bp[n_seg], bp_cov[n_seg], bp_bin[sum n_bp]): break points per segment, their coverage, their bins in segment order"""
        n = self.shape()[0]
        n_bp, cov, total = np.zeros(n, np.int32), np.zeros(n, np.int32), C.c_int64(0)
        check(load().hhx_correct_detect(self.h, float(median_cov_ratio), float(region_len_ratio), int(min_region_cutoff), ptr(n_bp), ptr(cov),
                                        C.byref(total)))
        bins = np.empty(total.value, np.int32)
        check(load().hhx_correct_fetch_break_points(self.h, ptr(bins) if bins.size else None))
        return n_bp, cov, bins

    def break_(self, seg, bp_off, bp_pos, zero):
        seg, bp_pos = np.ascontiguousarray(seg, np.int32), np.ascontiguousarray(bp_pos, np.int32)
        bp_off, zero = np.ascontiguousarray(bp_off, np.int64), np.ascontiguousarray(zero, np.uint8)
        check(load().hhx_correct_break(self.h, len(seg), ptr(seg), ptr(bp_off), ptr(bp_pos), ptr(zero)))


class ContigRemap(Handle):
    """hhx_remap: (original contig id, position) -> (corrected contig id, position - break offset) in place on device arrays."""
    _release = 'hhx_remap_destroy'

    def __init__(self, off, break_pos, new_id):
        off, break_pos, new_id = (np.ascontiguousarray(a, np.int32) for a in (off, break_pos, new_id))
        self.h = new_handle('hhx_remap_create', len(off) - 1, ptr(off), ptr(break_pos) if break_pos.size else None, ptr(new_id) if new_id.size else None)

    def apply(self, n, id_ptr, pos_ptr):
        check(load().hhx_remap_apply(self.h, int(n), C.c_void_p(id_ptr), C.c_void_p(pos_ptr)))
