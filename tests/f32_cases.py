"""Shapes of the float32 kernel tests (test_f32_exact_gpu.py, test_glue_exact_gpu.py), kept apart from the GPU modules so that
test_glue_refs_cpu.py can check the integer rule's precondition for every one of them without a GPU.

Integer rule: activations in {-4..4}, weights and gradients in {-2..2}, stored as float32.  Every product is an integer of magnitude <= 8
and every partial sum of n of them one of magnitude <= 8 n; below 2^24 every such integer is a float32, so any summation order gives the
exact result.  n = K (forward, data gradient), n = M (weight gradient: all positions, whatever the split), n = rows (column sums),
n = B (the head's weight gradient).
"""
INT_A, INT_W = 4, 2                         # largest |activation|, largest |weight| / |gradient| of the integer rule
LIMIT = 2 ** 24

D_CONVS = [(8, 1), (16, 3), (32, 5), (48, 7), (64, 9)]   # (output channels, kernel) of D.layers.0-4 (model.py:105-109)
G_LAYERS = [(128, 256, 5), (256, 256, 7), (256, 64, 5)]  # (Cin, Cout, K): the three distinct Conv1d geometries of G (model.py:49-77)


def d_dims(T):
    dims, H, W = [(64, T, 4)], 64, T
    for co, k in D_CONVS:
        H, W = H - k + 1, W - k + 1
        dims.append((H, W, co))
    return dims


# ---------------------------------------------------------------------------------------------- nele_conv_gemm
# (tag, B, Hout, Wout, C, N, KH, KW, dgrad): a valid convolution of a [B][Hout + KH - 1][Wout + KW - 1][C] window; dgrad: the window is the
# zero-bordered output gradient of a C <- N layer and the weights are its flipped ones
def gemm_cases():
    out = []
    # every TN (N <= 16, <= 32, <= 48, else the grid-y walk over 64-column blocks): N = 20 leaves a partial 16-column tile, N = 80 a partial
    # second grid-y block, N = 256 four blocks.  M = 2 * 5 * 37 = 370: a partial last block for every TM
    for N in (4, 8, 16, 20, 32, 48, 64, 80, 256):
        out.append(('N%d' % N, 2, 5, 37, 8, N, 3, 3, False))
    # G's Conv1d layers (H = 1) and their data gradients at B = 2, T = 24 and 40
    for T in (24, 40):
        for cin, cout, k in G_LAYERS:
            out.append(('G%dx%dx%d.T%d' % (cin, cout, k, T), 2, 1, T, cin, cout, 1, k, False))
            out.append(('G%dx%dx%d.T%d.dgrad' % (cin, cout, k, T), 2, 1, T, cout, cin, 1, k, True))
    # D.layers.0 (1 x 1, 4 -> 8) at T = 24, 40; D.layers.1-4 at T = 52 (Wout < 64: the span kernel declines them) and their data gradients
    for T in (24, 40):
        out.append(('D0.T%d' % T, 2, 64, T, 4, 8, 1, 1, False))
    dims = d_dims(52)
    for l in (1, 2, 3, 4):
        (Hi, Wi, Ci), (Ho, Wo, co), k = dims[l], dims[l + 1], D_CONVS[l][1]
        out.append(('D%d.T52' % l, 2, Ho, Wo, Ci, co, k, k, False))
        out.append(('D%d.T52.dgrad' % l, 2, Hi, Wi, co, Ci, k, k, True))
    # K = 36 is no multiple of the 8-wide K step; seglen = 12: a float4 ends exactly on the segment boundary
    out.append(('K36', 2, 6, 29, 4, 12, 3, 3, False))
    return out


# Linear-shaped problems (KH = KW = 1, C = 16) for the rows-per-block rule of nele_conv_gemm, derived from the host rule
#   TM = 4 iff ceil(M / 256) ny >= 512, else TM = 2 iff ceil(M / 128) ny >= 512, else TM = 1, ny = ceil(N / 64):
#   ny = 1 (N <= 64): TM = 2 from ceil(M / 128) >= 512, M >= 511 * 128 + 1 = 65 409; TM = 4 from M >= 511 * 256 + 1 = 130 817
#   ny = 4 (N = 256): TM = 2 from ceil(M / 128) >= 128, M >= 127 * 128 + 1 = 16 257; TM = 4 from M >= 127 * 256 + 1 = 32 513
# (N, M, TM expected); every M leaves a partial last block (M mod 64 != 0).  N = 8, 20, 48, 256 are TN = 1, 2, 3, 4: all twelve kernels.
def gemm_tm_cases():
    out = []
    for N in (8, 20, 48):
        out += [(N, 65407, 1), (N, 65411, 2), (N, 130815, 2), (N, 130819, 4)]
    out += [(256, 16255, 1), (256, 16259, 2), (256, 32511, 2), (256, 32515, 4)]
    return out


def gemm_tm(M, N):
    """the rule above, restated (not read from the kernel)"""
    ny = (N + 63) // 64
    if -(-M // 256) * ny >= 512:
        return 4
    return 2 if -(-M // 128) * ny >= 512 else 1


# ---------------------------------------------------------------------------------------------- nele_conv_span
# (tag, C, N, K): D.layers.1-4 forward, their data gradients (channels swapped) and the layer-0-shaped data gradient 8 -> 4 (1 x 1).
# nele_conv_span_supported by hand, for every layer below at every width of SPAN_WIDTHS (all >= 64):
#   N <= 64; seglen = K C = 24, 80, 224, 432 | 48, 160, 336, 576 | 8: multiples of 8; C a multiple of 4;
#   maxrun = ceil(256 / Wout) + 1 = 5 (Wout = 64, 65, 67), 3 (255), 2 (256, 257) <= 8;
#   LDS floats = 256 C + maxrun (K - 1) C <= 256 * 64 + 5 * 8 * 64 = 18 944 -> 75 776 bytes <= 76 KiB = 77 824;
#   KH seglen = Ktot and KW C = seglen by construction.
SPAN_LAYERS = [('D1', 8, 16, 3), ('D2', 16, 32, 5), ('D3', 32, 48, 7), ('D4', 48, 64, 9),
               ('D1.dgrad', 16, 8, 3), ('D2.dgrad', 32, 16, 5), ('D3.dgrad', 48, 32, 7), ('D4.dgrad', 64, 48, 9), ('D0.dgrad', 8, 4, 1)]
# exactly four runs per block (64), runs that straddle rows (65, 67), one or two runs (255, 256, 257)
SPAN_WIDTHS = [64, 65, 67, 255, 256, 257]
SPAN_B = 3                                  # a block's runs cross an utterance boundary (Hout = 3 or 4)


def span_hout(Wout):
    """3 or 4 rows: M = 3 Hout Wout is no multiple of 256 for any width but 256 (M = 2304 = 9 * 256, the exact-fit case)"""
    return 4 if Wout in (65, 255) else 3


# ---------------------------------------------------------------------------------------------- nele_conv_wgrad
# (tag, B, Hout, Wout, C, Cvalid, N, KH, KW, pad): pad = zero border of the output-gradient buffer (D: k - 1 on every side; G: None = K - 1 rows
# of END padding on the time axis)
def wgrad_cases():
    out = []
    for T in (40, 85):
        dims = d_dims(T)
        for l in (1, 2, 3, 4):
            (Hi, Wi, Ci), (Ho, Wo, co), k = dims[l], dims[l + 1], D_CONVS[l][1]
            out.append(('D%d.T%d' % (l, T), 2, Ho, Wo, Ci, Ci, co, k, k, k - 1))
        for cin, cout, k in G_LAYERS:                     # M = 80 (one split) and 170
            out.append(('G%dx%dx%d.T%d' % (cin, cout, k, T), 2, 1, T, cin, cin, cout, 1, k, None))
    # M = 8193 = 16 * 512 + 1: 17 splits, the last one holds a single row
    out.append(('last-split-1-row', 1, 3, 2731, 8, 8, 16, 3, 3, 0))
    # M = 8195: the last split holds three rows
    out.append(('last-split-3-rows', 1, 5, 1639, 8, 8, 16, 3, 3, 0))
    # the pointwise kernel (1 x 1, C = 4, N = 4 or 8; D.layers.0 has 3 valid channels of 4): 1, 5 and 71 (> 64, capped) splits of 512 rows
    for N in (4, 8):
        for M in (300, 2100, 512 * 70 + 3):
            out.append(('pointwise.N%d.M%d' % (N, M), 1, 1, M, 4, 3, N, 1, 1, 0))
    return out


# ---------------------------------------------------------------------------------------------- glue
COLSUM_SHAPES = [(r, c) for r in (1, 15, 16, 17, 1000) for c in (1, 64, 65, 256)]
MLP_WGRAD_B = [1, 7, 8, 9, 17]
MLP_WGRAD_NK = [(64, 64), (16, 64), (3, 16)]


def integer_rule_bounds():
    """(tag, largest possible |sum|) of every integer-rule case of the two GPU modules"""
    out = []
    for tag, B, Ho, Wo, C, N, KH, KW, dgrad in gemm_cases():
        out.append(('gemm.' + tag, INT_A * INT_W * KH * KW * C))
    for N, M, tm in gemm_tm_cases():
        out.append(('gemm.tm.N%d.M%d' % (N, M), INT_A * INT_W * 16))
    for tag, C, N, K in SPAN_LAYERS:
        out.append(('span.' + tag, INT_A * INT_W * K * K * C))
    for tag, B, Ho, Wo, C, Cv, N, KH, KW, pad in wgrad_cases():
        out.append(('wgrad.' + tag, INT_A * INT_W * B * Ho * Wo + INT_A * INT_W))       # + the value accumulated onto
    for r, c in COLSUM_SHAPES:
        out.append(('colsum.%dx%d' % (r, c), INT_A * r + INT_A))
    for B in MLP_WGRAD_B:
        out.append(('mlp_wgrad.B%d' % B, INT_A * INT_W * B))
    return out
