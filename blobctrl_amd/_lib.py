"""ctypes binding of libblobctrl_hip.so (the C ABI declared in include/blobctrl_hip.h).

The product path has NO fallback: if the shared library is missing or fails to load, importing any compute entry
point raises.  Build it with `python __graft_entry__.py` (hipcc --offload-arch=gfx950).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# BLOBCTRL_HIP_LIB points at another build of the SAME C ABI (A/B measurements of kernel variants); default = the in-tree build
LIB_PATH = os.environ.get("BLOBCTRL_HIP_LIB") or os.path.join(_HERE, "libblobctrl_hip.so")

A_DENSE, A_CONV3X3 = 0, 1
ACT_NONE, ACT_GELU, ACT_GEGLU, ACT_SILU, ACT_QUICK_GELU = 0, 1, 2, 3, 4
OUT_F16, OUT_F16_T, OUT_F32 = 0, 1, 2
TILE_NAMES = ["auto", "256x128", "128x128_s3", "128x128_s2", "256x64_s2", "256x64_s3", "128x64", "64x64", "halo128x160", "wreg128x160",
              "gw64x128", "gw64x256", "gw64x320", "g256x256"]
TILE_HALO = 8
TILE_WREG = 9
TILE_GW64x128, TILE_GW64x256, TILE_GW64x320 = 10, 11, 12
TILE_G256 = 13                       # gemm256.hip: 256 x 256 tiles, 8 waves, 8-phase LDS-DMA pipeline, persistent workgroups
GW_TILES = {TILE_GW64x128: 2, TILE_GW64x256: 4, TILE_GW64x320: 5}      # configuration -> 16-column tiles per wave (BN = 64 NT)


class BcGemm(C.Structure):
    """Mirror of `struct BcGemm` (include/blobctrl_hip.h) - keep field order identical."""
    _fields_ = [
        ("A", C.c_void_p), ("A2", C.c_void_p), ("a_mode", C.c_int),
        ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
        ("lda", C.c_int), ("lda2", C.c_int), ("C1", C.c_int), ("Cin", C.c_int),
        ("Hin", C.c_int), ("Win", C.c_int), ("Hv", C.c_int), ("Wv", C.c_int),
        ("Hout", C.c_int), ("Wout", C.c_int), ("stride", C.c_int), ("conv_nopad_lo", C.c_int),
        ("W", C.c_void_p), ("ldw", C.c_int),
        ("bias", C.c_void_p), ("rowvec", C.c_void_p), ("ld_rowvec", C.c_int), ("rows_per_batch", C.c_int),
        ("rowvec_idx", C.c_void_p), ("rowvec_step", C.c_int),
        ("act", C.c_int), ("colscale", C.c_void_p), ("alpha", C.c_float),
        ("alpha_dev", C.c_void_p), ("alpha_idx", C.c_void_p), ("alpha_bstride", C.c_int),
        ("R", C.c_void_p), ("ldr", C.c_int),
        ("R2", C.c_void_p), ("ldr2", C.c_int), ("r2_xmin", C.c_int), ("r2_bmod", C.c_int), ("out_w", C.c_int),
        ("out_mode", C.c_int), ("C", C.c_void_p), ("ldc", C.c_int),
        ("splitk", C.c_int), ("slab", C.c_void_p), ("gn_tot", C.c_void_p), ("tile_cfg", C.c_int),
        ("a_affine", C.c_void_p), ("a_act", C.c_int),
        ("a_tot1", C.c_void_p), ("a_tot2", C.c_void_p),
        ("a_gamma", C.c_void_p), ("a_beta", C.c_void_p), ("a_groups", C.c_int), ("a_eps", C.c_float),
        ("ln_colsum", C.c_void_p), ("ln_eps", C.c_float),
        ("C_t", C.c_void_p), ("ldc_t", C.c_int), ("n_t0", C.c_int),
        ("w_bstride", C.c_longlong), ("vec_bstride", C.c_int), ("sm_group", C.c_int), ("sm_valid", C.c_int), ("sm_keep", C.c_int),
        ("S", C.c_void_p), ("S2", C.c_void_p), ("lds", C.c_int), ("lds2", C.c_int), ("S1", C.c_int), ("Cs", C.c_int),
    ]


FAMILIES = ("gemm", "gemm_fast", "conv_halo", "conv_wreg", "gemm_wreg", "gemm256")       # BC_FAMILY_*: the kernel family of a resolved BcGemm


class BcGemmInfo(C.Structure):
    """Mirror of `struct BcGemmInfo` (include/blobctrl_hip.h): how the library launches a BcGemm (bc_gemm_resolve)."""
    _fields_ = [("family", C.c_int), ("tile_cfg", C.c_int), ("bm", C.c_int), ("bn", C.c_int), ("splitk", C.c_int), ("n_out", C.c_int),
                ("slab_elems", C.c_longlong), ("stat_rows", C.c_int), ("gn_finalize_fits", C.c_int), ("kernel", C.c_char * 64)]


_SIGNATURES = {
    "bc_last_error": (C.c_char_p, []),
    "bc_version": (C.c_int, []),
    "bc_device_info": (C.c_int, [C.POINTER(C.c_int)]),
    "bc_gemm": (C.c_int, [C.POINTER(BcGemm), C.c_void_p]),
    "bc_sizeof_gemm": (C.c_int, []),
    "bc_gemm_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                               C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bc_gemm_resolve": (C.c_int, [C.POINTER(BcGemm), C.POINTER(BcGemmInfo)]),
    "bc_conv_halo_eligible": (C.c_int, [C.c_int] * 8),
    "bc_conv_halo_max_chunks": (C.c_int, []),
    "bc_conv_wreg_pack": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "bc_conv_wreg_pack_sc": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "bc_conv_wreg_sc_eligible": (C.c_int, [C.c_int] * 7),
    "bc_conv_wreg_pack_host": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "bc_gemm_wreg_pack": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "bc_gemm_wreg_stream_elems": (C.c_longlong, [C.c_int, C.c_int]),
    "bc_gemm_wreg_eligible": (C.c_int, [C.c_int] * 5),
    "bc_gemm256_eligible": (C.c_int, [C.c_int] * 7),
    "bc_gn_stats": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "bc_gn_finalize": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bc_gn_apply_fused": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                    C.c_void_p]),
    "bc_memset_zero": (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p]),
    "bc_dup_halves": (C.c_int, [C.c_void_p, C.c_longlong] * 6 + [C.c_void_p]),
    "bc_freeu": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                           C.c_void_p, C.c_void_p, C.c_void_p]),
    "bc_gn_apply": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                              C.c_void_p, C.c_void_p]),
    "bc_softmax_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "bc_gaussian_sample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "bc_layernorm": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p,
                               C.c_int, C.c_void_p]),
    "bc_attention": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                               C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_longlong, C.c_longlong,
                               C.c_longlong, C.c_float, C.c_void_p]),
    "bc_attention_causal": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_longlong, C.c_longlong,
                                      C.c_longlong, C.c_float, C.c_void_p]),
    "bc_attention_build": (C.c_int, [C.c_int] * 6),
    "bc_embed_tokens": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                  C.c_void_p]),
    "bc_splat_scores": (C.c_int, [C.POINTER(C.c_double), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "bc_splat_maps": (C.c_int, [C.POINTER(C.c_double), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bc_alpha_composite": (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p]),
    "bc_splat_from_scores": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_longlong,
                                       C.c_longlong, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "bc_resize_bilinear": (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "bc_pack_rgb8": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "bc_assemble_input": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                    C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "bc_assemble_input_im2col": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_void_p, C.c_void_p]),
    "bc_assemble_input_scaled": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "bc_assemble_input_im2col_scaled": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                  C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "bc_timestep_embedding": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "bc_timestep_embedding_table": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "bc_timestep_embedding_cond": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bc_timestep_embedding_table_cond": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bc_silu": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    "bc_cfg_scheduler_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int,
                                        C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "bc_cfg_scheduler_step_noise": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int,
                                              C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "bc_cfg_scheduler_step3": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int,
                                         C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "bc_scheduler_step_single": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                           C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "bc_nchw_to_nhwc_f16": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "bc_nhwc_to_nchw": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "bc_add_cls_pos": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "bc_patchify": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "bc_rowchain_supported": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "bc_rowchain_stream_frags": (C.c_longlong, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "bc_rowchain": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float,
                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                              C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_float,
                              C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "bc_rowchain_sum": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bc_rowchain_kv_frags": (C.c_longlong, [C.c_int]),
    "bc_rowchain_pack_kv": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "bc_ctx_fold": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bc_rowchain_midx": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float,
                                   C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]),
    # ---- plan runtime (plan.hip)
    "bc_plan_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "bc_plan_destroy": (C.c_int, [C.c_void_p]),
    "bc_plan_segment": (C.c_int, [C.c_void_p, C.c_char_p]),
    "bc_plan_find_segment": (C.c_int, [C.c_void_p, C.c_char_p]),
    "bc_plan_new_event": (C.c_int, [C.c_void_p]),
    "bc_plan_add_gemm": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(BcGemm)]),
    "bc_plan_add_op": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.c_int]),
    "bc_plan_set_slab": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "bc_plan_enable": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "bc_plan_num_launches": (C.c_int, [C.c_void_p, C.c_int]),
    "bc_step": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_int]),
    "bc_plan_capture": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_int]),
    "bc_plan_release": (C.c_int, [C.c_void_p, C.c_int]),
    "bc_plan_capture_loop": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p)]),
    "bc_plan_run_timed": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_float)]),
    "bc_plan_run_timed_kernels": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "bc_plan_run_marked": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_float)]),
    "bc_plan_save": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int]),
    "bc_plan_load": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    "bc_plan_buffer": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_longlong)]),
    "bc_graph_begin": (C.c_int, [C.c_void_p]),
    "bc_graph_end": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "bc_graph_launch": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bc_graph_destroy": (C.c_int, [C.c_void_p]),
    "bc_event_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "bc_event_create_sync": (C.c_int, [C.POINTER(C.c_void_p)]),
    "bc_stream_wait_event": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bc_event_record": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bc_event_elapsed_ms": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]),
    "bc_event_destroy": (C.c_int, [C.c_void_p]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES.keys())

# Entry points of include/blobctrl_vae.h (the tiled-VAE driver's blend / crop / scatter launch).  A table of its own: these are host-driven
# helpers, not recordable plan ops, and EXPORTED_SYMBOLS stays the list of include/blobctrl_hip.h.
VAE_SIGNATURES = {
    "bc_vae_tile_blend": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
}
VAE_TILE_DECODE, VAE_TILE_ENCODE = 0, 1

# Entry points of include/blobctrl_requests.h (request batches whose requests run their own schedules).  A table of its own, as that
# header is one of its own; unlike the VAE helpers these ARE recordable plan ops (REQUEST_OPS below).
REQUEST_SIGNATURES = {
    "bc_assemble_input_requests": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                             C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "bc_assemble_input_im2col_requests": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                    C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "bc_timestep_embedding_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "bc_scheduler_step_requests": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                             C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
}

# Entry points of include/blobctrl_sam.h (the Segment-Anything path of blobctrl_amd/sam.py).  A table of its own like the request forms;
# all are recordable (SAM_OPS below), but SAM segments live in-process only - nothing of them is written to a plan file.
_ATTN_RELPOS_ARGS = [C.c_void_p] * 4 + [C.c_int] * 11 + [C.c_longlong] * 4 + [C.c_float] + [C.c_void_p] * 3 + [C.c_void_p]
SAM_SIGNATURES = {
    "bc_attention_relpos": (C.c_int, _ATTN_RELPOS_ARGS),
    "bc_window_partition": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "bc_window_unpartition": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "bc_add_pos": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "bc_add_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "bc_act_rows": (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p]),
    "bc_bilinear_resize_f32": (C.c_int, [C.c_void_p] + [C.c_int] * 8 + [C.c_float, C.c_void_p, C.c_void_p]),
    "bc_sam_tokens": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float,
                                C.c_void_p, C.c_void_p]),
    "bc_sam_masks": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
}
# ... and the entry points behind batched prompts / SamAutomaticMaskGenerator, declared in the same header: a table of their own
# (SAM_BATCH_OPS below), recordable and in-process only like SAM_OPS.  bc_mask_stats_chunks is a host query, not a launch.
SAM_BATCH_SIGNATURES = {
    "bc_sam_tokens_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_float, C.c_void_p, C.c_void_p]),
    "bc_mask_stats": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
}
SAM_HOST_SIGNATURES = {"bc_mask_stats_chunks": (C.c_int, [C.c_int, C.c_int])}

# Entry points of include/blobctrl_masks.h (connected components and small-region removal, blobctrl_amd/masks.py).  A table of its own:
# these are DIRECT launches on the caller's stream - no BC_OP_* code, in none of the op tables below, never recorded into a plan.
_MASK_REMOVE_ARGS = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
MASK_SIGNATURES = {
    "bc_mask_label": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "bc_mask_remove_small": (C.c_int, _MASK_REMOVE_ARGS + [C.c_void_p]),
    "bc_mask_remove_small_phase": (C.c_int, _MASK_REMOVE_ARGS + [C.c_int, C.c_void_p]),
}
MASK_HOLES, MASK_ISLANDS = 0, 1
MASK_REGION_PHASES = 5                # launch groups of bc_mask_remove_small (BC_MASK_REGION_PHASES)

# Entry points of include/blobctrl_edit.h (an edit's inputs built on the device, blobctrl_amd/edit_inputs.py).  A table of its own, as for
# the masks: DIRECT launches on the caller's stream - no BC_OP_* code, in none of the op tables below, never recorded into a plan.
EDIT_SIGNATURES = {
    "bc_ellipse_cover": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "bc_ellipse_paint": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "bc_mask_row_extents": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "bc_mask_cutout": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
}
EDIT_MAX_DIM = 16384                  # largest H and W those entry points take (BC_EDIT_MAX_DIM)

# Entry points of include/blobctrl_resample.h (Pillow's 8-bit resize on the device, blobctrl_amd/resample.py).  A table of its own, as for
# the edit inputs: DIRECT launches on the caller's stream - no BC_OP_* code, in none of the op tables below, never recorded into a plan.
RESAMPLE_SIGNATURES = {
    "bc_resample_horizontal": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                         C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "bc_resample_vertical": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                       C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
}

# Entry points of include/blobctrl_overlay.h (zoomed edits: a mask's bounds, Pillow's Gaussian blur, the paste-back; blobctrl_amd/overlay.py).
# A table of its own, as for the resize: DIRECT launches on the caller's stream - no BC_OP_* code, in no op table, never recorded.
_BLUR_ARGS = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
OVERLAY_SIGNATURES = {
    "bc_box_blur3_rows": (C.c_int, _BLUR_ARGS),
    "bc_box_blur3_cols": (C.c_int, _BLUR_ARGS),
    "bc_mask_bounds": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bc_overlay_composite": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_void_p, C.c_void_p]),
}
BLUR_MAX_R = 63                       # largest integer box radius of the blur launches (BC_BLUR_MAX_R)

# Entry point of include/blobctrl_ip.h (the IP-Adapter image cross-attention, accumulated onto attn2's text attention in place).  A table
# of its own; a recordable plan op (IP_OPS below), in-process only like the SAM ops.
IP_SIGNATURES = {
    "bc_attention_ip": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
}
ATTENTION_IP_MAX_T = 64               # image tokens per launch (BC_ATTENTION_IP_MAX_T)
# The two kernels behind bc_attention_ip by name (include/blobctrl_ip.h): which one the library picks for a shape, and a launch of a named
# one.  Plain entry points for measurements and tests - no BC_OP_* code, in no op table, never recorded into a plan.
IP_PATH_SIGNATURES = {
    "bc_attention_ip_path": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "bc_attention_ip_with": (C.c_int, [C.c_int] + IP_SIGNATURES["bc_attention_ip"][1]),
}
ATTENTION_IP_SCALAR, ATTENTION_IP_TILES = 0, 1

# Entry points of include/blobctrl_ip_mask.h (ip_adapter_masks: one softmax per image, each weighted by its mask).  Tables of their own:
# the masked attention is a recordable plan op (IP_MASK_OPS below), in-process only like bc_attention_ip ...
IP_MASK_SIGNATURES = {
    "bc_attention_ip_masked": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
}
# ... and the rest are DIRECT launches and plain entry points - no BC_OP_* code, in no op table, never recorded into a plan: the bicubic
# downsampling of a mask to one attention level, and the masked kernels by name
IP_MASK_DIRECT_SIGNATURES = {
    "bc_ip_mask_downsample": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                        C.c_void_p]),
    "bc_attention_ip_masked_path": (C.c_int, [C.c_int] * 5),
    "bc_attention_ip_masked_with": (C.c_int, [C.c_int] + IP_MASK_SIGNATURES["bc_attention_ip_masked"][1]),
}

# Entry points of include/blobctrl_tiny_vae.h (the AutoencoderTiny decoder, blobctrl_amd/tiny_vae.py).  bc_tiny_conv3x3 takes the struct
# below; the recordable plan ops (TINY_VAE_OPS below, in-process only) are its flat form and the latent prologue.
class BcTinyConvArgs(C.Structure):
    """Mirror of `struct bc_tiny_conv_args` (include/blobctrl_tiny_vae.h) - keep field order identical."""
    _fields_ = [("x", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("skip", C.c_void_p), ("out", C.c_void_p),
                ("B", C.c_int), ("H", C.c_int), ("W", C.c_int), ("Ci", C.c_int), ("Co", C.c_int),
                ("up", C.c_int), ("relu", C.c_int), ("out_mode", C.c_int)]


TINY_VAE_SIGNATURES = {
    "bc_tiny_conv3x3_flat": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 8 + [C.c_void_p]),
    "bc_tiny_latents_in": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
}
TINY_VAE_DIRECT_SIGNATURES = {"bc_tiny_conv3x3": (C.c_int, [C.POINTER(BcTinyConvArgs), C.c_void_p])}
TINY_OUT_F16, TINY_OUT_IMAGE, TINY_OUT_U8 = 0, 1, 2

# Entry points of include/blobctrl_pag.h (perturbed-attention guidance: the identity attention of the perturbed images and the step of a
# PAG plan).  A table of its own; both are recordable plan ops (PAG_OPS below), in-process only like the IP-Adapter ops.
PAG_SIGNATURES = {
    "bc_attention_identity": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "bc_pag_scheduler_step": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 3 + [C.c_void_p] + [C.c_int] * 3 + [C.c_void_p, C.c_int, C.c_void_p]),
}

# Entry points of include/blobctrl_blend.h (masked edits: the step of a blend plan and the mask at latent resolution).  A table of its
# own; both are recordable plan ops (BLEND_OPS below), in-process only like the PAG ops.
BLEND_SIGNATURES = {
    "bc_blend_scheduler_step": (C.c_int, [C.c_void_p] * 10 + [C.c_int] * 3 + [C.c_void_p] + [C.c_int] * 3 + [C.c_void_p, C.c_int, C.c_void_p]),
    "bc_blend_mask": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
}

# Recordable entry points of the plan runtime: name -> BC_OP_* code (include/blobctrl_hip.h).  The argument kinds of an op are derived
# from its ctypes signature above (stream excluded): p pointer, i int, f float, l long long - the same strings plan.hip checks.
OPS = {"bc_gemm": 0, "bc_gn_stats": 1, "bc_gn_finalize": 2, "bc_gn_apply_fused": 3, "bc_gn_apply": 4, "bc_layernorm": 5,
       "bc_attention": 6, "bc_attention_causal": 7, "bc_assemble_input": 8, "bc_timestep_embedding": 9,
       "bc_timestep_embedding_table": 10, "bc_cfg_scheduler_step": 11, "bc_embed_tokens": 12, "bc_softmax_rows": 13,
       "bc_patchify": 14, "bc_add_cls_pos": 15, "bc_silu": 16, "bc_nchw_to_nhwc_f16": 17, "bc_nhwc_to_nchw": 18,
       "bc_gaussian_sample": 19, "bc_rowchain": 22, "bc_assemble_input_im2col": 23, "bc_memset_zero": 24,
       "bc_rowchain_midx": 25, "bc_rowchain_pack_kv": 26, "bc_rowchain_sum": 27, "bc_ctx_fold": 28, "bc_dup_halves": 29,
       "bc_cfg_scheduler_step_noise": 30, "bc_cfg_scheduler_step3": 31,
       "bc_assemble_input_scaled": 32, "bc_assemble_input_im2col_scaled": 33, "bc_scheduler_step_single": 34,
       "bc_timestep_embedding_table_cond": 35, "bc_timestep_embedding_cond": 36, "bc_freeu": 37}
# ... and those of include/blobctrl_requests.h (plan file version 8); `op_code` looks a name up in both tables
REQUEST_OPS = {"bc_scheduler_step_requests": 38, "bc_assemble_input_requests": 39, "bc_assemble_input_im2col_requests": 40,
               "bc_timestep_embedding_rows": 41}
# ... and those of include/blobctrl_sam.h
SAM_OPS = {"bc_attention_relpos": 42, "bc_window_partition": 43, "bc_window_unpartition": 44, "bc_add_pos": 45, "bc_add_rows": 46,
           "bc_act_rows": 47, "bc_bilinear_resize_f32": 48, "bc_sam_tokens": 49, "bc_sam_masks": 50}
SAM_BATCH_OPS = {"bc_sam_tokens_batch": 51, "bc_mask_stats": 52}
# ... and that of include/blobctrl_ip.h: extension headers continue from BC_OP_COUNT (53), the base header's enum is closed
IP_OPS = {"bc_attention_ip": 53}
# ... and that of include/blobctrl_ip_mask.h, an enum of its own behind BC_OP_IP_END (54, which stays no op)
IP_MASK_OPS = {"bc_attention_ip_masked": 55}
_OP_TABLES = (OPS, REQUEST_OPS, SAM_OPS, SAM_BATCH_OPS, IP_OPS)
# _OP_TABLES is the list up to BC_OP_IP_END and stays as it is; tables of headers that start an enum of their own behind it go here, and
# `op_code` reads both
_OP_TABLES_BEYOND = (IP_MASK_OPS,)
# ... and those of include/blobctrl_tiny_vae.h, again an enum of its own behind BC_OP_IP_MASK_END (56, which stays no op)
TINY_VAE_OPS = {"bc_tiny_conv3x3_flat": 57, "bc_tiny_latents_in": 58}
_OP_TABLES_TINY_VAE = (TINY_VAE_OPS,)
# ... and those of include/blobctrl_pag.h, again an enum of its own behind BC_OP_TINY_VAE_END (59, which stays no op)
PAG_OPS = {"bc_attention_identity": 60, "bc_pag_scheduler_step": 61}
_OP_TABLES_PAG = (PAG_OPS,)
# ... and those of include/blobctrl_blend.h, again an enum of its own behind BC_OP_PAG_END (62, which stays no op)
BLEND_OPS = {"bc_blend_scheduler_step": 63, "bc_blend_mask": 64}
_OP_TABLES_BLEND = (BLEND_OPS,)
OP_SIGNAL, OP_WAIT = 20, 21
CHAIN_IN, CHAIN_MID, CHAIN_OUT, CHAIN_OUT_FF, CHAIN_OUT_TAIL, CHAIN_MIDX, CHAIN_OUT_FFP = 0, 1, 2, 3, 4, 5, 6
GN_TOT_WORDS = 6                      # 64-bit words per (image, channel) of a GroupNorm statistics table (include/blobctrl_hip.h)
_KIND = {C.c_void_p: "p", C.c_int: "i", C.c_float: "f", C.c_longlong: "l", C.c_char_p: "p"}


def op_code(name):
    """BC_OP_* code of a recordable entry point."""
    for table in _OP_TABLES + _OP_TABLES_BEYOND + _OP_TABLES_TINY_VAE + _OP_TABLES_PAG + _OP_TABLES_BLEND:
        if name in table:
            return table[name]
    raise KeyError(name)


def op_signature(name):
    """Argument kinds of a recordable entry point without its trailing stream argument."""
    args = (_SIGNATURES.get(name) or REQUEST_SIGNATURES.get(name) or SAM_SIGNATURES.get(name) or SAM_BATCH_SIGNATURES.get(name) or
            IP_SIGNATURES.get(name) or IP_MASK_SIGNATURES.get(name) or TINY_VAE_SIGNATURES.get(name) or PAG_SIGNATURES.get(name) or
            BLEND_SIGNATURES[name])[1][:-1]
    return "".join("p" if (a not in _KIND) else _KIND[a] for a in args)


class BcPlanBuffer(C.Structure):
    _fields_ = [("name", C.c_char_p), ("address", C.c_void_p), ("bytes", C.c_longlong), ("host_data", C.c_void_p)]

_lib = None


class BlobCtrlHipError(RuntimeError):
    pass


def load():
    """Load the HIP library (once).  Raises BlobCtrlHipError if it is missing - there is no CPU fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BlobCtrlHipError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  blobctrl_amd has no CPU fallback.")
    # PyTorch (the device-memory / stream provider of this package) ships its own libamdhip64; if this library were loaded first
    # it would pull in the system copy and the process would end up with TWO HIP runtimes - the second one then reports "no
    # ROCm-capable device".  Importing torch first makes the loader bind our HIP calls to the runtime torch already uses.
    try:
        import torch  # noqa: F401
    except ImportError:   # pragma: no cover - plain C / ctypes use without PyTorch: the system HIP runtime is the only one
        pass
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:   # pragma: no cover
        raise BlobCtrlHipError(f"failed to load {LIB_PATH}: {e}") from e
    for name, (res, args) in list(_SIGNATURES.items()) + list(VAE_SIGNATURES.items()) + list(REQUEST_SIGNATURES.items()) + \
            list(SAM_SIGNATURES.items()) + list(SAM_BATCH_SIGNATURES.items()) + list(SAM_HOST_SIGNATURES.items()) + \
            list(MASK_SIGNATURES.items()) + list(EDIT_SIGNATURES.items()) + list(RESAMPLE_SIGNATURES.items()) + \
            list(IP_SIGNATURES.items()) + list(IP_PATH_SIGNATURES.items()) + list(OVERLAY_SIGNATURES.items()) + \
            list(IP_MASK_SIGNATURES.items()) + list(IP_MASK_DIRECT_SIGNATURES.items()) + list(TINY_VAE_SIGNATURES.items()) + \
            list(TINY_VAE_DIRECT_SIGNATURES.items()) + list(PAG_SIGNATURES.items()) + list(BLEND_SIGNATURES.items()):
        fn = getattr(lib, name)          # AttributeError => symbol missing from the build
        fn.restype = res
        fn.argtypes = args
    if lib.bc_sizeof_gemm() != C.sizeof(BcGemm):
        raise BlobCtrlHipError(f"BcGemm layout mismatch: C {lib.bc_sizeof_gemm()} vs ctypes {C.sizeof(BcGemm)}")
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().bc_last_error()
        raise BlobCtrlHipError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")
