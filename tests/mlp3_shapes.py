"""The M x K x N table of dr_mlp3_fwd cases: run on the GPU by tests/test_gpu_widths.py
(test_mlp3_shape_sweep), their GEMM routes pinned on the host by tests/test_gemm_plan_host.py."""
# ---------------------------------------------------------------------------
# dr_mlp3_fwd: GEMM routes by M x K x N.  Layers: L0 = Linear over [h | z]
# (AM_PLAIN, K = in_h + in_z), L3 / L6 = Linear over SiLU(LayerNorm(.))
# (AM_LNSILU, K = h1 / h2).  The route of every layer of every case (kernel
# instantiation, grid, dynamic LDS) is pinned without a GPU by
# tests/test_gemm_plan_host.py, which asks gemm.hip's planner (gemm_plan) about
# these shapes; the comments below say why a case is here.  "16 x 16 vec" =
# k_gemm_skinny<16, 16, ..., VEC = true> and so on; `how` = the h operand's layout.
# ---------------------------------------------------------------------------
MLP3_SHAPES = [
    # (M, in_h, in_z, h1, h2, n_out, how)
    # one row, N = 1, no z segment (lin, not lin2): all three layers 16 x 16 vec, one row tile with 15 dead rows;
    # L6 has a single live column
    (1, 64, 0, 32, 32, 1, "packed"),
    # every K off 4 (67 = 61 + 6, 30, 22): the float4-row test (rows_aligned) fails on K % 4 (and ksplitA % 4) for all three layers ->
    # k_gemm_skinny<16, 16, ..., VEC = false>, L3 / L6 with its scalar LN-SiLU prologue; two row tiles, the second
    # with one live row; N = 41 leaves a 9-column tail tile
    (17, 61, 6, 30, 22, 41, "packed"),
    # K % 4 == 0 everywhere: 16 x 16 vec on all layers (L3 K = 36 and L6 K = 52 staged, KP = 44 / 60)
    (16, 64, 64, 36, 52, 255, "packed"),
    # ldh = 65: lda % 4 != 0 although K % 4 == 0 -> L0 non-vec (L3 / L6 read the packed scratch: vec)
    (16, 64, 64, 36, 52, 255, "ldh65"),
    # h one float past a 16-byte boundary: aligned16(A) fails -> L0 non-vec
    (16, 64, 64, 36, 52, 255, "offset1"),
    # FULL widths just past 64 rows: t16 = 5 x 13 = 65 (L0, L3), 5 x 16 = 80 (L6) <= 640 -> 16-row tiles; 65 leaves
    # a one-row tail tile, 127 a 15-row one
    (65, 600, 1024, 200, 200, 255, "packed"),
    (127, 600, 1024, 200, 200, 255, "packed"),
    # L6: t16 = 13 x 64 = 832 > 640 -> 64-row tiles (4 row tiles, the last with 8 live rows); tiles16 = 4 x 64 = 256
    # is not > 256 and maxM > 64 -> 64 x 16; L0 / L3 t16 = 169 -> 16-row tiles
    (200, 600, 1024, 200, 200, 1024, "packed"),
    # L0: M in 128..512, K = 1624 >= 1024, tiles32 = 8 x 17 = 136 >= 112, K % 8 == 0 -> launch_wk (no planes, fp32);
    # L3: LayerNorm over K = 520: t16 = 16 x 13 = 208 -> 16 x 16 tiles, staged (K / 4 = 130 <= 256 lanes x vectors,
    # (16 + 16) x 520 floats of LDS)
    (256, 600, 1024, 520, 200, 255, "packed"),
    # L0: K = 1620, K % 8 != 0 -> wk_ok fails -> launch_tile2<32, 32, 64, false, false, 4> (vec: K % 4 == 0)
    (256, 600, 1020, 520, 200, 255, "packed"),
    # L0: M = 1040 >= 1024, tiles = 17 x 16 = 272 >= 256 -> `tall`, K = 128 < 1024 -> launch_tile2<64, 64, 32> with
    # partial row (1040 = 16 x 64 + 16) and column (1000 = 15 x 64 + 40) tiles; L3: LayerNorm over K = 1000 at
    # M > 64 (no a_out: not tall_ln_ok); with N = 40, t16 = 65 x 3 = 195 <= 640 keeps 16-row tiles, where K = 1000
    # is still staged (K / 4 = 250 <= 256, 32 x 1000 <= SK_LN_MAXF); L6: N = 8, K = 40
    (1040, 64, 64, 1000, 40, 8, "packed"),
    # the same with h2 = 200: L3 t16 = 65 x 13 = 845 > 640 -> 64 x 16 tiles (17 x 4 = 68 tiles of 64 x 64: not
    # `tall`), where K = 1000 is past the staged limit (K / 4 <= 64) and the LDS-row limit (K / 4 <= 128, 64 x 1000
    # floats > SK_LN_MAXF): row statistics from global memory, LN-SiLU applied on the fly
    (1040, 64, 64, 1000, 200, 8, "packed"),
    # the staged boundary of the 16-row tile.  L3: K = 1024 is the last staged K (K / 4 = 256, 32 x 1032 floats);
    # L6: K = 1028 is the first on the direct path with the LayerNorm rows in LDS (16 x 1032 floats = 66048 bytes:
    # over 64 KB, the launch that opts in to more dynamic LDS)
    (16, 64, 0, 1024, 1028, 16, "packed"),
    # L3: K = 2048 is the last K with the LayerNorm rows in LDS (K / 4 = 512, 16 x 2056 floats); L6: K = 2052 takes
    # its LayerNorm statistics from global memory
    (16, 64, 0, 2048, 2052, 16, "packed"),
]
