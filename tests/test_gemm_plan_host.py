"""gemm_plan (csrc/gemm.hip) on the host: the route of a batch -- kernel
instantiation, grid, block, dynamic LDS, split count, packed problems -- through
dr_internal_gemm_plan, without a GPU.

EXPECT is profiles/gemm_plan_routes_parent.txt as literals: the launches the
commit before the planner made for the same batches, recorded from its
gemm.hip with the launch macro replaced by a recorder.  A threshold change
shows up here as a changed line."""
import ctypes

import pytest

INT_MAX = 2 ** 31 - 1
G_NT, G_NN, G_TN = 0, 1, 2
PLAIN, LNSILU, CONV, CONV_SRC, LNBWD, STEBWD = range(6)
SAMPLE, ACTOR = 1, 2
DR_E_INVALID = 1001
# dr_internal_gemm_plan's flag word
A2, LN, AOUT, PRE, WS, PLANES, A16, BF16, W2, OUT_CONV, ADDEND, ACC, BIAS = (
    1, 2, 4, 8, 16, 32, 64, 128, 1024, 2048, 4096, 8192, 16384)
STEP_INTS = 21
(F_LEGACY, F_SKINNY, F_TILE, F_TILE_B16, F_WK, F_WKS3, F_LN_SAMPLE, F_S3_TALL, F_LN_ROWS, F_FINISH) = range(10)


def prob(M, N, K, flags=0, lda=None, lda2=0, ksA=INT_MAX, ldb=None, ldy=None, C=0, R=0, na=0, epi=0, ws=0, np_=0,
         mis0=0, mis1=0, ld_aout=None):
    """One problem as the hook's 17 ints (mis0 / mis1: misalignment nibbles A A2 W Y ln_g ln_b a_out pre / wsplit A16
    bias z_out); ws > 0 gives split-K scratch of that many floats, np_ > 0 weight planes of that many rows."""
    flags |= (epi << 8) | (WS if ws else 0) | (PLANES if np_ else 0)
    lda = K if lda is None else lda
    return [M, N, K, lda, lda2, ksA, K if ldb is None else ldb, N if ldy is None else ldy, C, R, na,
            flags, ws, np_, mis0, mis1, lda if ld_aout is None else ld_aout]


def _b(x):
    return "true" if x else "false"


def _kernel(s):
    (fam, bm, bn, kc, nw, amode, a_km, b_kn, vec, epi, bf16, a16) = s[:12]
    return {
        F_LEGACY: f"k_gemm<{bm},{bn},{amode},{_b(a_km)},{_b(b_kn)}>",
        F_SKINNY: f"k_gemm_skinny<{bm},{bn},{amode},{_b(b_kn)},{_b(vec)},{epi}>",
        F_TILE: f"k_gemm_tile<{bm},{bn},{kc},{_b(a_km)},{_b(b_kn)},{_b(vec)},{nw}>",
        F_TILE_B16: f"k_gemm_tile_b16<{bm},{bn},{nw}>",
        F_WK: f"k_gemm_wk<{bm},{bn},{nw},2,1>",
        F_WKS3: f"k_gemm_wks3<{1 if bf16 else 3},1,{nw},{bm // 16},{_b(a16)}>",
        F_LN_SAMPLE: f"k_ln_gemm_sample<{kc}>",
        F_S3_TALL: "s3_tall",
        F_LN_ROWS: f"k_ln_silu_rows<{kc}>",
        F_FINISH: "k_splitk_finish",
    }[fam]


def plan_steps(lay, amode, probs):
    """(steps as lists of ints, None) or (None, (code, message))."""
    from dreamer_amd import _lib
    f = _lib.load().dr_internal_gemm_plan
    f.restype = ctypes.c_int
    flat = [v for p in probs for v in p] or [0]
    arr = (ctypes.c_int * len(flat))(*flat)
    out = (ctypes.c_int * (STEP_INTS * 10))()
    msg = ctypes.create_string_buffer(256)
    n = f(ctypes.c_int(lay), ctypes.c_int(amode), ctypes.c_int(len(probs)), arr, out, ctypes.c_int(10), msg,
          ctypes.c_int(256))
    if n < 0:
        return None, (-n, msg.value.decode())
    return [list(out[STEP_INTS * k:STEP_INTS * (k + 1)]) for k in range(n)], None


def route(lay, amode, probs):
    """The plan in the recorded table's form, one launch per ';'-separated entry:
    kernel g<grid> b<block> l<LDS bytes> i<int kernel arguments> p<problem>a<A operand: 1 the caller's, 7 its a_out
    after the LN pre-pass>w<split-K scratch passed>.  The a / w tokens are worked out here from the plan's ln_pre and
    no_ws: this pins what the planner asks for, not the batch the executor then builds from it (gemm_run's
    after_ln_rows and scratch withholding), which only the GPU tests run."""
    steps, err = plan_steps(lay, amode, probs)
    if err:
        return f"E {err[0]} {err[1]}"
    ln_pre = any(s[0] == F_LN_ROWS for s in steps)
    out = []
    for s in steps:
        fam, mask = s[0], s[12]
        gx, gy, gz, block, lds, splits, npack, no_ws = s[13:21]
        idx = [i for i in range(4) if mask >> i & 1]
        if fam == F_S3_TALL:
            p = probs[idx[0]]
            out.append(f"s3_tall p{idx[0]} part{p[12] if p[11] & WS else 0}")
            continue
        ints = {F_SKINNY: [npack], F_TILE: [splits, npack], F_TILE_B16: [splits], F_WK: [1, npack], F_WKS3: [npack],
                F_FINISH: [splits]}.get(fam, [])
        toks = [_kernel(s), f"g{gx},{gy},{gz}", f"b{block}", f"l{lds}"] + [f"i{v}" for v in ints]
        if fam != F_LN_ROWS:
            for i in idx:
                has_ws = bool(probs[i][11] & WS) and not no_ws
                toks.append(f"p{i}a{7 if ln_pre else 1}w{int(has_ws)}")
        else:
            toks.append(f"p{idx[0]}")
        out.append(" ".join(toks))
    return " ; ".join(out) if out else "-"


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------
def mlp3_layers(M, in_h, in_z, h1, h2, n_out, how):
    """dr_mlp3_fwd's three launches (engine.hip mlp3) for a tests/mlp3_shapes.py MLP3_SHAPES case."""
    K0 = in_h + in_z
    ldh = in_h + 1 if how == "ldh65" else in_h
    l0 = prob(M, h1, K0, BIAS | (A2 if in_z else 0), lda=ldh, lda2=in_z, ksA=in_h if in_z else INT_MAX,
              mis0=4 if how == "offset1" else 0)
    return [(PLAIN, l0), (LNSILU, prob(M, h2, h1, BIAS | LN)), (LNSILU, prob(M, n_out, h2, BIAS | LN))]


def _cases():
    from mlp3_shapes import MLP3_SHAPES
    C = {}
    for shape in MLP3_SHAPES:
        for li, (amode, p) in zip((0, 3, 6), mlp3_layers(*shape)):
            C["mlp3 " + "-".join(str(v) for v in shape) + f" L{li}"] = (G_NT, amode, [p])
    lnb = lambda M, N, K, **kw: prob(M, N, K, LN | PRE | AOUT, **kw)
    ste = lambda M, N, K, C_=32, **kw: prob(M, N, K, PRE, C=C_, **kw)
    # the staged backward prologues at the update phase's shapes
    C["lnbwd B256 N600 K200"] = (G_NT, LNBWD, [prob(256, 600, 200, LN | PRE | AOUT | ACC)])
    C["lnbwd B256 N200 K200"] = (G_NT, LNBWD, [lnb(256, 200, 200)])
    C["stebwd B256 N200 K1024"] = (G_NT, STEBWD, [ste(256, 200, 1024)])
    C["stebwd B512 N200 K1024"] = (G_NT, STEBWD, [ste(512, 200, 1024)])
    # t16 = 640 | 641: 16-row tiles | 64-row tiles
    C["t16 640 plain"] = (G_NT, PLAIN, [prob(10240, 16, 64)])
    C["t16 641 plain"] = (G_NT, PLAIN, [prob(10256, 16, 64)])
    for name, amode, mk in (("plain", PLAIN, lambda M, N: prob(M, N, 64)), ("lnsilu", LNSILU, lambda M, N: prob(M, N, 64, LN)),
                            ("lnbwd", LNBWD, lambda M, N: lnb(M, N, 64))):
        three = [mk(160, 256) for _ in range(3)]
        C[f"t16 640 {name} x4"] = (G_NT, amode, three + [mk(160, 256)])
        C[f"t16 641 {name} x4"] = (G_NT, amode, three + [mk(112, 368)])
    smp = lambda M, N: prob(M, N, 64, epi=SAMPLE, C=32, R=N // 32)
    C["t16 640 sample"] = (G_NT, PLAIN, [smp(2560, 128)])
    C["t16 641 sample x2"] = (G_NT, PLAIN, [smp(2560, 128), smp(16, 32)])
    # tiles16 256 | 257: 16 | 32 columns
    for name, amode, fl in (("plain", PLAIN, 0), ("lnsilu", LNSILU, LN)):
        C[f"tiles16 256 {name}"] = (G_NT, amode, [prob(64, 1024, 64, fl)])
        C[f"tiles16 257 {name}"] = (G_NT, amode, [prob(64, 1024, 64, fl), prob(16, 16, 64, fl)])
    # tiles32 111 | 112 (K >= 1024) and 255 | 256 (K >= 512)
    C["tiles32 111"] = (G_NT, PLAIN, [prob(128, 864, 1024), prob(96, 32, 1024)])
    C["tiles32 112"] = (G_NT, PLAIN, [prob(128, 864, 1024), prob(128, 32, 1024)])
    for ws in (0, 1):
        w = lambda M, N: 4 * M * N * ws
        C[f"tiles32 255 ws{ws}"] = (G_NT, PLAIN, [prob(480, 544, 512, ws=w(480, 544))])
        C[f"tiles32 256 ws{ws}"] = (G_NT, PLAIN, [prob(512, 512, 512, ws=w(512, 512))])
    # maxM
    C["maxM 64"] = (G_NT, PLAIN, [prob(64, 200, 64)])
    C["maxM 65"] = (G_NT, PLAIN, [prob(65, 200, 64)])
    C["maxM 127"] = (G_NT, PLAIN, [prob(127, 1624, 1624)])
    C["maxM 128"] = (G_NT, PLAIN, [prob(128, 1624, 1624)])
    for ws in (0, 1):
        C[f"maxM 512 ws{ws}"] = (G_NT, PLAIN, [prob(512, 200, 1624, ws=4 * 512 * 200 * ws)])
        C[f"maxM 513 ws{ws}"] = (G_NT, PLAIN, [prob(513, 200, 1624, ws=4 * 513 * 200 * ws)])
    C["maxM 1023"] = (G_NT, PLAIN, [prob(1023, 1024, 200)])
    C["maxM 1024"] = (G_NT, PLAIN, [prob(1024, 1024, 200)])
    # minK
    C["minK 511"] = (G_NT, PLAIN, [prob(512, 512, 511)])
    C["minK 1023"] = (G_NT, PLAIN, [prob(256, 520, 1023)])
    C["minK 1023 planes"] = (G_NT, PLAIN, [prob(256, 520, 1024, np_=544), prob(256, 520, 1023, np_=544)])
    C["minK 504 planes"] = (G_NT, PLAIN, [prob(512, 512, 504, np_=512, lda=512)])
    C["minK 508"] = (G_NT, PLAIN, [prob(512, 512, 508)])
    C["minK 512"] = (G_NT, PLAIN, [prob(512, 512, 512)])
    C["minK 1020"] = (G_NT, PLAIN, [prob(256, 520, 1020)])
    C["minK 1024"] = (G_NT, PLAIN, [prob(256, 520, 1024)])
    C["minK 1016 1024"] = (G_NT, PLAIN, [prob(256, 520, 1024), prob(256, 520, 1016)])
    # K % 8 (wave-K), K % 4 (tile kernel, float4 rows), K % 4 != 0 (scalar rows)
    C["K 1624"] = (G_NT, PLAIN, [prob(256, 520, 1624)])
    C["K 1620"] = (G_NT, PLAIN, [prob(256, 520, 1620)])
    C["K 1622"] = (G_NT, PLAIN, [prob(256, 520, 1622)])
    # split-K scratch: none, for four splits, for two
    for name, f in (("none", 0), ("x4", 4), ("x2", 2)):
        C[f"splitk {name}"] = (G_NT, PLAIN, [prob(256, 200, 1620, ws=f * 256 * 200) for _ in range(3)])
        C[f"splitk bf16 {name}"] = (G_NT, PLAIN, [prob(256, 200, 1624, BF16, ws=f * 256 * 200) for _ in range(3)])
    C["splitk some"] = (G_NT, PLAIN, [prob(256, 200, 1620, ws=4 * 256 * 200), prob(256, 200, 1620)])
    C["splitk tall"] = (G_NT, PLAIN, [prob(1024, 200, 1624, ws=4 * 1024 * 200)])
    C["splitk tall bf16"] = (G_NT, PLAIN, [prob(1024, 200, 1624, BF16, ws=4 * 1024 * 200)])
    # weight planes (the wave-K split3 kernel), one row short, bf16, A16 for all | some
    C["planes K200"] = (G_NT, PLAIN, [prob(256, 1624, 200, np_=1632)])
    C["planes K200 short"] = (G_NT, PLAIN, [prob(256, 1624, 200, np_=1631)])
    C["planes K512"] = (G_NT, PLAIN, [prob(256, 1624, 512, np_=1632, ws=4 * 256 * 1624)])
    C["planes K1624 x3"] = (G_NT, PLAIN, [prob(256, 200, 1624, np_=224) for _ in range(3)])
    C["planes K1624 short"] = (G_NT, PLAIN, [prob(256, 200, 1624, np_=224), prob(256, 200, 1624, np_=223)])
    C["planes bf16"] = (G_NT, PLAIN, [prob(256, 1624, 200, BF16, np_=1632)])
    C["planes bf16 a16"] = (G_NT, PLAIN, [prob(256, 1624, 200, BF16 | A16, np_=1632) for _ in range(2)])
    C["planes bf16 a16 some"] = (G_NT, PLAIN, [prob(256, 1624, 200, BF16 | A16, np_=1632), prob(256, 1624, 200, BF16, np_=1632)])
    C["planes bf16 a16 lda"] = (G_NT, PLAIN, [prob(256, 1624, 200, BF16 | A16, lda=204, np_=1632)])
    C["no planes bf16"] = (G_NT, PLAIN, [prob(256, 1624, 200, BF16)])
    # the split3 tall GEMM: problems that qualify one by one, the rest as a batch
    tall = lambda ok, ws=0: prob(3840, 200, 200, np_=256 if ok else 255, ws=ws)
    C["s3 tall x1"] = (G_NT, PLAIN, [tall(True, 4 * 3840 * 200)])
    C["s3 tall x1 not"] = (G_NT, PLAIN, [tall(False)])
    C["s3 tall x2 one"] = (G_NT, PLAIN, [tall(False), tall(True)])
    C["s3 tall x4 two"] = (G_NT, PLAIN, [tall(True), tall(False), tall(True), tall(False)])
    C["s3 tall x4 all"] = (G_NT, PLAIN, [tall(True) for _ in range(4)])
    C["s3 tall bf16"] = (G_NT, PLAIN, [prob(3840, 200, 200, BF16, np_=256)])
    # the LN-SiLU pre-pass of tall products, and each clause that rules it out
    tl = lambda M=3840, K=200, fl=LN | AOUT | BIAS, **kw: prob(M, 200, K, fl, **kw)
    C["tall_ln"] = (G_NT, LNSILU, [tl()])
    C["tall_ln K1024 x2"] = (G_NT, LNSILU, [tl(K=1024), tl(K=256)])
    C["tall_ln planes"] = (G_NT, LNSILU, [tl(np_=256)])
    C["tall_ln M1023"] = (G_NT, LNSILU, [tl(M=1023)])
    C["tall_ln no a_out"] = (G_NT, LNSILU, [tl(fl=LN | BIAS)])
    C["tall_ln K202"] = (G_NT, LNSILU, [tl(K=202)])
    C["tall_ln K1028"] = (G_NT, LNSILU, [tl(K=1028)])
    C["tall_ln K0"] = (G_NT, LNSILU, [tl(K=0)])
    C["tall_ln A2"] = (G_NT, LNSILU, [tl(fl=LN | AOUT | BIAS | A2, lda2=100, ksA=100)])
    C["tall_ln lda201"] = (G_NT, LNSILU, [tl(lda=201)])
    C["tall_ln A off"] = (G_NT, LNSILU, [tl(mis0=4)])
    C["tall_ln gamma off"] = (G_NT, LNSILU, [tl(mis0=4 << 16)])
    C["tall_ln beta off"] = (G_NT, LNSILU, [tl(mis0=4 << 20)])
    C["tall_ln a_out off"] = (G_NT, LNSILU, [tl(mis0=4 << 24)])
    C["tall_ln ld_aout 201"] = (G_NT, LNSILU, [tl(ld_aout=201)])
    C["tall_ln epi"] = (G_NT, LNSILU, [prob(3840, 6, 200, LN | AOUT | BIAS, epi=ACTOR, na=3)])
    C["tall_ln rows 2^31 lda"] = (G_NT, LNSILU, [tl(lda=559244)])
    C["tall_ln rows 2^31 ld_aout"] = (G_NT, LNSILU, [tl(ld_aout=559244)])
    C["tall_ln rows below 2^31"] = (G_NT, LNSILU, [tl(ld_aout=559240)])
    C["tall_ln x2 one"] = (G_NT, LNSILU, [tl(), tl(M=1023)])
    # the sampler head
    C["ln_sample"] = (G_NT, LNSILU, [prob(256, 1024, 200, LN | BIAS, epi=SAMPLE, C=32, R=32)])
    C["ln_sample K256"] = (G_NT, LNSILU, [prob(16, 64, 256, LN | BIAS, epi=SAMPLE, C=32, R=2)])
    C["ln_sample C16"] = (G_NT, LNSILU, [prob(256, 1024, 200, LN | BIAS, epi=SAMPLE, C=16, R=64)])
    C["ln_sample K260"] = (G_NT, LNSILU, [prob(256, 1024, 260, LN | BIAS, epi=SAMPLE, C=32, R=32)])
    C["sample plain M65"] = (G_NT, PLAIN, [prob(65, 1024, 200, BIAS, epi=SAMPLE, C=32, R=32)])
    C["actor"] = (G_NT, LNSILU, [prob(256, 6, 200, LN | BIAS, epi=ACTOR, na=3)])
    C["actor M1024"] = (G_NT, LNSILU, [prob(1024, 6, 200, LN | BIAS, epi=ACTOR, na=3)])
    # gemm_launch's errors
    C["err count 0"] = (G_NT, PLAIN, [])
    C["err count 5"] = (G_NT, PLAIN, [prob(16, 16, 16) for _ in range(5)])
    C["err negative"] = (G_NT, PLAIN, [prob(16, -1, 16)])
    C["err sampler C3"] = (G_NT, PLAIN, [prob(16, 30, 16, epi=SAMPLE, C=3, R=10)])
    C["err actor N"] = (G_NT, PLAIN, [prob(16, 7, 16, epi=ACTOR, na=3)])
    C["err epi M4097"] = (G_NT, PLAIN, [prob(4097, 6, 16, epi=ACTOR, na=3)])
    C["err epi NN"] = (G_NN, PLAIN, [prob(16, 6, 16, epi=ACTOR, na=3)])
    C["err lnbwd K1028"] = (G_NT, LNBWD, [lnb(256, 200, 1028)])
    C["err lnbwd K260 rows64"] = (G_NT, LNBWD, [lnb(1024, 200, 260)])
    C["err lnbwd pre off"] = (G_NT, LNBWD, [lnb(256, 200, 200, mis0=8 << 28)])
    C["err stebwd rows64"] = (G_NT, STEBWD, [ste(1024, 200, 256)])
    C["err stebwd C24"] = (G_NT, STEBWD, [ste(256, 200, 240, C_=24)])
    C["err lnbwd offsets"] = (G_NT, LNBWD, [lnb(4096, 16, 64, lda=262144)])
    C["err amode"] = (G_NT, 6, [prob(16, 16, 16)])
    C["lnbwd K256 rows64"] = (G_NT, LNBWD, [lnb(1024, 200, 256)])
    C["lnbwd K1024"] = (G_NT, LNBWD, [lnb(256, 200, 1024)])
    # NN (input gradients), TN (weight gradients) and the legacy tiles either side of work = 256 * 1024
    C["nn skinny"] = (G_NN, PLAIN, [prob(256, 200, 64, ldb=200)])
    C["nn tile"] = (G_NN, PLAIN, [prob(512, 512, 512, ldb=512, ws=4 * 512 * 512)])
    C["tn tile"] = (G_TN, PLAIN, [prob(200, 1624, 3840, lda=200, ldb=1624)])
    C["tn tile x4 ws"] = (G_TN, PLAIN, [prob(200, 200, 3840, lda=200, ldb=200, ws=4 * 200 * 200) for _ in range(4)])
    for name, lay, amode, fl in (("nn", G_NN, PLAIN, OUT_CONV), ("tn", G_TN, PLAIN, OUT_CONV), ("conv", G_NT, CONV, 0),
                                 ("conv_src", G_NT, CONV_SRC, 0)):
        C[f"legacy {name} below"] = (lay, amode, [prob(512, 508, 64, fl, lda=512, ldb=512)])
        C[f"legacy {name} at"] = (lay, amode, [prob(512, 512, 64, fl, lda=512, ldb=512)])
    C["legacy x2 at"] = (G_NT, CONV, [prob(512, 256, 64), prob(256, 512, 64)])
    # 32-bit element offsets either side of 2^30
    C["offsets below"] = (G_NT, PLAIN, [prob(4096, 64, 64, lda=262140)])
    C["offsets at"] = (G_NT, PLAIN, [prob(4096, 64, 64, lda=262144)])
    C["offsets W at"] = (G_NT, PLAIN, [prob(64, 4096, 64, ldb=262144)])
    C["offsets tile below"] = (G_NT, PLAIN, [prob(1024, 1024, 4096, lda=262140)])
    C["offsets tile at"] = (G_NT, PLAIN, [prob(1024, 1024, 4096, lda=262144)])
    return C


EXPECT = {
    'mlp3 1-64-0-32-32-1-packed L0':
        'k_gemm_skinny<16,16,0,false,true,0> g8,1,1 b512 l8192 i0 p0a1w0',
    'mlp3 1-64-0-32-32-1-packed L3':
        'k_gemm_skinny<16,16,1,false,true,0> g8,1,1 b512 l8192 i0 p0a1w0',
    'mlp3 1-64-0-32-32-1-packed L6':
        'k_gemm_skinny<16,16,1,false,true,0> g8,1,1 b512 l8192 i0 p0a1w0',
    'mlp3 17-61-6-30-22-41-packed L0':
        'k_gemm_skinny<16,16,0,false,false,0> g8,1,1 b512 l8192 i0 p0a1w0',
    'mlp3 17-61-6-30-22-41-packed L3':
        'k_gemm_skinny<16,16,1,false,false,0> g8,1,1 b512 l8192 i0 p0a1w0',
    'mlp3 17-61-6-30-22-41-packed L6':
        'k_gemm_skinny<16,16,1,false,false,0> g8,1,1 b512 l8192 i0 p0a1w0',
    'mlp3 16-64-64-36-52-255-packed L0':
        'k_gemm_skinny<16,16,0,false,true,0> g8,1,1 b512 l8192 i0 p0a1w0',
    'mlp3 16-64-64-36-52-255-packed L3':
        'k_gemm_skinny<16,16,1,false,true,0> g8,1,1 b512 l8192 i0 p0a1w0',
    'mlp3 16-64-64-36-52-255-packed L6':
        'k_gemm_skinny<16,16,1,false,true,0> g16,1,1 b512 l8192 i0 p0a1w0',
    'mlp3 16-64-64-36-52-255-ldh65 L0':
        'k_gemm_skinny<16,16,0,false,false,0> g8,1,1 b512 l8192 i0 p0a1w0',
    'mlp3 16-64-64-36-52-255-ldh65 L3':
        'k_gemm_skinny<16,16,1,false,true,0> g8,1,1 b512 l8192 i0 p0a1w0',
    'mlp3 16-64-64-36-52-255-ldh65 L6':
        'k_gemm_skinny<16,16,1,false,true,0> g16,1,1 b512 l8192 i0 p0a1w0',
    'mlp3 16-64-64-36-52-255-offset1 L0':
        'k_gemm_skinny<16,16,0,false,false,0> g8,1,1 b512 l8192 i0 p0a1w0',
    'mlp3 16-64-64-36-52-255-offset1 L3':
        'k_gemm_skinny<16,16,1,false,true,0> g8,1,1 b512 l8192 i0 p0a1w0',
    'mlp3 16-64-64-36-52-255-offset1 L6':
        'k_gemm_skinny<16,16,1,false,true,0> g16,1,1 b512 l8192 i0 p0a1w0',
    'mlp3 65-600-1024-200-200-255-packed L0':
        'k_gemm_skinny<16,16,0,false,true,0> g72,1,1 b512 l8192 i0 p0a1w0',
    'mlp3 65-600-1024-200-200-255-packed L3':
        'k_gemm_skinny<16,16,1,false,true,0> g72,1,1 b512 l25600 i0 p0a1w0',
    'mlp3 65-600-1024-200-200-255-packed L6':
        'k_gemm_skinny<16,16,1,false,true,0> g80,1,1 b512 l25600 i0 p0a1w0',
    'mlp3 127-600-1024-200-200-255-packed L0':
        'k_gemm_skinny<16,16,0,false,true,0> g104,1,1 b512 l8192 i0 p0a1w0',
    'mlp3 127-600-1024-200-200-255-packed L3':
        'k_gemm_skinny<16,16,1,false,true,0> g104,1,1 b512 l25600 i0 p0a1w0',
    'mlp3 127-600-1024-200-200-255-packed L6':
        'k_gemm_skinny<16,16,1,false,true,0> g128,1,1 b512 l25600 i0 p0a1w0',
    'mlp3 200-600-1024-200-200-1024-packed L0':
        'k_gemm_skinny<16,16,0,false,true,0> g176,1,1 b512 l8192 i0 p0a1w0',
    'mlp3 200-600-1024-200-200-1024-packed L3':
        'k_gemm_skinny<16,16,1,false,true,0> g176,1,1 b512 l25600 i0 p0a1w0',
    'mlp3 200-600-1024-200-200-1024-packed L6':
        'k_gemm_skinny<64,16,1,false,true,0> g256,1,1 b512 l64000 i0 p0a1w0',
    'mlp3 256-600-1024-520-200-255-packed L0':
        'k_gemm_wk<32,32,4,2,1> g136,1,1 b256 l0 i1 i0 p0a1w0',
    'mlp3 256-600-1024-520-200-255-packed L3':
        'k_gemm_skinny<16,16,1,false,true,0> g208,1,1 b512 l66560 i0 p0a1w0',
    'mlp3 256-600-1024-520-200-255-packed L6':
        'k_gemm_skinny<16,16,1,false,true,0> g256,1,1 b512 l25600 i0 p0a1w0',
    'mlp3 256-600-1020-520-200-255-packed L0':
        'k_gemm_tile<32,32,64,false,false,true,4> g136,1,1 b256 l0 i1 i0 p0a1w0',
    'mlp3 256-600-1020-520-200-255-packed L3':
        'k_gemm_skinny<16,16,1,false,true,0> g208,1,1 b512 l66560 i0 p0a1w0',
    'mlp3 256-600-1020-520-200-255-packed L6':
        'k_gemm_skinny<16,16,1,false,true,0> g256,1,1 b512 l25600 i0 p0a1w0',
    'mlp3 1040-64-64-1000-40-8-packed L0':
        'k_gemm_tile<64,64,32,false,false,true,4> g272,1,1 b256 l0 i1 i0 p0a1w0',
    'mlp3 1040-64-64-1000-40-8-packed L3':
        'k_gemm_skinny<16,16,1,false,true,0> g200,1,1 b512 l128000 i0 p0a1w0',
    'mlp3 1040-64-64-1000-40-8-packed L6':
        'k_gemm_skinny<16,16,1,false,true,0> g72,1,1 b512 l8192 i0 p0a1w0',
    'mlp3 1040-64-64-1000-200-8-packed L0':
        'k_gemm_tile<64,64,32,false,false,true,4> g272,1,1 b256 l0 i1 i0 p0a1w0',
    'mlp3 1040-64-64-1000-200-8-packed L3':
        'k_gemm_skinny<64,16,1,false,true,0> g224,1,1 b512 l32768 i0 p0a1w0',
    'mlp3 1040-64-64-1000-200-8-packed L6':
        'k_gemm_skinny<16,16,1,false,true,0> g72,1,1 b512 l25600 i0 p0a1w0',
    'mlp3 16-64-0-1024-1028-16-packed L0':
        'k_gemm_skinny<16,16,0,false,true,0> g64,1,1 b512 l8192 i0 p0a1w0',
    'mlp3 16-64-0-1024-1028-16-packed L3':
        'k_gemm_skinny<16,16,1,false,true,0> g72,1,1 b512 l132096 i0 p0a1w0',
    'mlp3 16-64-0-1024-1028-16-packed L6':
        'k_gemm_skinny<16,16,1,false,true,0> g8,1,1 b512 l66048 i0 p0a1w0',
    'mlp3 16-64-0-2048-2052-16-packed L0':
        'k_gemm_skinny<16,16,0,false,true,0> g128,1,1 b512 l8192 i0 p0a1w0',
    'mlp3 16-64-0-2048-2052-16-packed L3':
        'k_gemm_skinny<16,16,1,false,true,0> g136,1,1 b512 l131584 i0 p0a1w0',
    'mlp3 16-64-0-2048-2052-16-packed L6':
        'k_gemm_skinny<16,16,1,false,true,0> g8,1,1 b512 l8192 i0 p0a1w0',
    'lnbwd B256 N600 K200':
        'k_gemm_skinny<16,48,4,false,true,0> g208,1,1 b512 l51200 i0 p0a1w0',
    'lnbwd B256 N200 K200':
        'k_gemm_skinny<16,16,4,false,true,0> g208,1,1 b512 l25600 i0 p0a1w0',
    'stebwd B256 N200 K1024':
        'k_gemm_skinny<16,16,5,false,true,0> g208,1,1 b512 l132096 i0 p0a1w0',
    'stebwd B512 N200 K1024':
        'k_gemm_skinny<16,16,5,false,true,0> g416,1,1 b512 l132096 i0 p0a1w0',
    't16 640 plain':
        'k_gemm_skinny<16,32,0,false,true,0> g640,1,1 b512 l16384 i0 p0a1w0',
    't16 641 plain':
        'k_gemm_skinny<64,16,0,false,true,0> g168,1,1 b512 l32768 i0 p0a1w0',
    't16 640 plain x4':
        'k_gemm_skinny<16,32,0,false,true,0> g320,1,1 b512 l16384 i4 p0a1w0 p1a1w0 p2a1w0 p3a1w0',
    't16 641 plain x4':
        'k_gemm_skinny<64,16,0,false,true,0> g192,1,1 b512 l32768 i4 p0a1w0 p1a1w0 p2a1w0 p3a1w0',
    't16 640 lnsilu x4':
        'k_gemm_skinny<16,32,1,false,true,0> g320,1,1 b512 l16384 i4 p0a1w0 p1a1w0 p2a1w0 p3a1w0',
    't16 641 lnsilu x4':
        'k_gemm_skinny<64,16,1,false,true,0> g192,1,1 b512 l32768 i4 p0a1w0 p1a1w0 p2a1w0 p3a1w0',
    't16 640 lnbwd x4':
        'k_gemm_skinny<16,48,4,false,true,0> g240,1,1 b512 l24576 i4 p0a1w0 p1a1w0 p2a1w0 p3a1w0',
    't16 641 lnbwd x4':
        'k_gemm_skinny<64,16,4,false,true,0> g192,1,1 b512 l32768 i4 p0a1w0 p1a1w0 p2a1w0 p3a1w0',
    't16 640 sample':
        'k_gemm_skinny<16,32,0,false,true,1> g640,1,1 b512 l16384 i0 p0a1w0',
    't16 641 sample x2':
        'k_gemm_skinny<64,32,0,false,true,1> g168,1,1 b512 l65536 i2 p0a1w0 p1a1w0',
    'tiles16 256 plain':
        'k_gemm_skinny<16,16,0,false,true,0> g256,1,1 b512 l8192 i0 p0a1w0',
    'tiles16 257 plain':
        'k_gemm_skinny<16,32,0,false,true,0> g136,1,1 b512 l16384 i2 p0a1w0 p1a1w0',
    'tiles16 256 lnsilu':
        'k_gemm_skinny<16,16,1,false,true,0> g256,1,1 b512 l9216 i0 p0a1w0',
    'tiles16 257 lnsilu':
        'k_gemm_skinny<16,32,1,false,true,0> g136,1,1 b512 l16384 i2 p0a1w0 p1a1w0',
    'tiles32 111':
        'k_gemm_skinny<16,32,0,false,true,0> g224,1,1 b512 l16384 i2 p0a1w0 p1a1w0',
    'tiles32 112':
        'k_gemm_wk<32,32,4,2,1> g112,1,1 b256 l0 i1 i2 p0a1w0 p1a1w0',
    'tiles32 255 ws0':
        'k_gemm_skinny<64,16,0,false,true,0> g272,1,1 b512 l32768 i0 p0a1w0',
    'tiles32 256 ws0':
        'k_gemm_wk<32,32,4,2,1> g256,1,1 b256 l0 i1 i0 p0a1w0',
    'tiles32 255 ws1':
        'k_gemm_tile<64,64,32,false,false,true,4> g72,4,1 b256 l0 i4 i0 p0a1w1 ; k_splitk_finish g1020,1,1 b256 l0 i4 p0a1w1',
    'tiles32 256 ws1':
        'k_gemm_wk<32,32,4,2,1> g256,1,1 b256 l0 i1 i0 p0a1w0',
    'maxM 64':
        'k_gemm_skinny<16,16,0,false,true,0> g56,1,1 b512 l8192 i0 p0a1w0',
    'maxM 65':
        'k_gemm_skinny<16,16,0,false,true,0> g72,1,1 b512 l8192 i0 p0a1w0',
    'maxM 127':
        'k_gemm_skinny<64,16,0,false,true,0> g208,1,1 b512 l32768 i0 p0a1w0',
    'maxM 128':
        'k_gemm_wk<32,32,4,2,1> g208,1,1 b256 l0 i1 i0 p0a1w0',
    'maxM 512 ws0':
        'k_gemm_wk<32,32,4,2,1> g112,1,1 b256 l0 i1 i0 p0a1w0',
    'maxM 513 ws0':
        'k_gemm_skinny<16,32,0,false,true,0> g232,1,1 b512 l16384 i0 p0a1w0',
    'maxM 512 ws1':
        'k_gemm_wk<32,32,4,2,1> g112,1,1 b256 l0 i1 i0 p0a1w1',
    'maxM 513 ws1':
        'k_gemm_tile<64,64,64,false,false,true,8> g40,4,1 b512 l0 i4 i0 p0a1w1 ; k_splitk_finish g401,1,1 b256 l0 i4 p0a1w1',
    'maxM 1023':
        'k_gemm_skinny<64,16,0,false,true,0> g1024,1,1 b512 l32768 i0 p0a1w0',
    'maxM 1024':
        'k_gemm_tile<64,64,32,false,false,true,4> g256,1,1 b256 l0 i1 i0 p0a1w0',
    'minK 511':
        'k_gemm_skinny<64,16,0,false,false,0> g256,1,1 b512 l32768 i0 p0a1w0',
    'minK 1023':
        'k_gemm_skinny<16,32,0,false,false,0> g272,1,1 b512 l16384 i0 p0a1w0',
    'minK 1023 planes':
        'k_gemm_tile<32,32,64,false,false,false,4> g272,1,1 b256 l0 i1 i2 p0a1w0 p1a1w0',
    'minK 504 planes':
        'k_gemm_wks3<3,1,4,2,false> g256,1,1 b256 l0 i0 p0a1w0',
    'minK 508':
        'k_gemm_skinny<64,16,0,false,true,0> g256,1,1 b512 l32768 i0 p0a1w0',
    'minK 512':
        'k_gemm_wk<32,32,4,2,1> g256,1,1 b256 l0 i1 i0 p0a1w0',
    'minK 1020':
        'k_gemm_skinny<16,32,0,false,true,0> g272,1,1 b512 l16384 i0 p0a1w0',
    'minK 1024':
        'k_gemm_wk<32,32,4,2,1> g136,1,1 b256 l0 i1 i0 p0a1w0',
    'minK 1016 1024':
        'k_gemm_wk<32,32,4,2,1> g272,1,1 b256 l0 i1 i2 p0a1w0 p1a1w0',
    'K 1624':
        'k_gemm_wk<32,32,4,2,1> g136,1,1 b256 l0 i1 i0 p0a1w0',
    'K 1620':
        'k_gemm_tile<32,32,64,false,false,true,4> g136,1,1 b256 l0 i1 i0 p0a1w0',
    'K 1622':
        'k_gemm_tile<32,32,64,false,false,false,4> g136,1,1 b256 l0 i1 i0 p0a1w0',
    'splitk none':
        'k_gemm_tile<32,32,64,false,false,true,4> g168,1,1 b256 l0 i1 i3 p0a1w0 p1a1w0 p2a1w0',
    'splitk bf16 none':
        'k_gemm_tile_b16<32,32,4> g56,1,3 b256 l0 i1 p0a1w0 p1a1w0 p2a1w0',
    'splitk x4':
        'k_gemm_tile<32,32,64,false,false,true,4> g168,4,1 b256 l0 i4 i3 p0a1w1 p1a1w1 p2a1w1 ; k_splitk_finish g200,1,3 b256 l0 i4 p0a1w1 p1a1w1 p2a1w1',
    'splitk bf16 x4':
        'k_gemm_tile_b16<32,32,4> g56,4,3 b256 l0 i4 p0a1w1 p1a1w1 p2a1w1 ; k_splitk_finish g200,1,3 b256 l0 i4 p0a1w1 p1a1w1 p2a1w1',
    'splitk x2':
        'k_gemm_tile<32,32,64,false,false,true,4> g168,2,1 b256 l0 i2 i3 p0a1w1 p1a1w1 p2a1w1 ; k_splitk_finish g200,1,3 b256 l0 i2 p0a1w1 p1a1w1 p2a1w1',
    'splitk bf16 x2':
        'k_gemm_tile_b16<32,32,4> g56,2,3 b256 l0 i2 p0a1w1 p1a1w1 p2a1w1 ; k_splitk_finish g200,1,3 b256 l0 i2 p0a1w1 p1a1w1 p2a1w1',
    'splitk some':
        'k_gemm_tile<32,32,64,false,false,true,4> g112,1,1 b256 l0 i1 i2 p0a1w1 p1a1w0',
    'splitk tall':
        'k_gemm_tile<64,64,64,false,false,true,8> g64,4,1 b512 l0 i4 i0 p0a1w1 ; k_splitk_finish g800,1,1 b256 l0 i4 p0a1w1',
    'splitk tall bf16':
        'k_gemm_tile_b16<64,64,8> g64,4,1 b512 l0 i4 p0a1w1 ; k_splitk_finish g800,1,1 b256 l0 i4 p0a1w1',
    'planes K200':
        'k_gemm_wks3<3,1,4,2,false> g408,1,1 b256 l0 i0 p0a1w0',
    'planes K200 short':
        'k_gemm_skinny<64,16,0,false,true,0> g408,1,1 b512 l32768 i0 p0a1w0',
    'planes K512':
        'k_gemm_wks3<3,1,4,2,false> g408,1,1 b256 l0 i0 p0a1w0',
    'planes K1624 x3':
        'k_gemm_wks3<3,1,4,2,false> g168,1,1 b256 l0 i3 p0a1w0 p1a1w0 p2a1w0',
    'planes K1624 short':
        'k_gemm_wk<32,32,4,2,1> g112,1,1 b256 l0 i1 i2 p0a1w0 p1a1w0',
    'planes bf16':
        'k_gemm_wks3<1,1,4,1,false> g816,1,1 b256 l0 i0 p0a1w0',
    'planes bf16 a16':
        'k_gemm_wks3<1,1,4,1,true> g1632,1,1 b256 l0 i2 p0a1w0 p1a1w0',
    'planes bf16 a16 some':
        'k_gemm_wks3<1,1,4,1,false> g1632,1,1 b256 l0 i2 p0a1w0 p1a1w0',
    'planes bf16 a16 lda':
        'k_gemm_wks3<1,1,4,1,false> g816,1,1 b256 l0 i0 p0a1w0',
    'no planes bf16':
        'k_gemm_skinny<64,16,0,false,true,0> g408,1,1 b512 l32768 i0 p0a1w0',
    's3 tall x1':
        's3_tall p0 part3072000',
    's3 tall x1 not':
        'k_gemm_skinny<64,16,0,false,true,0> g784,1,1 b512 l32768 i0 p0a1w0',
    's3 tall x2 one':
        's3_tall p1 part0 ; k_gemm_skinny<64,16,0,false,true,0> g784,1,1 b512 l32768 i0 p0a1w0',
    's3 tall x4 two':
        's3_tall p0 part0 ; s3_tall p2 part0 ; k_gemm_tile<64,64,32,false,false,true,4> g480,1,1 b256 l0 i1 i2 p1a1w0 p3a1w0',
    's3 tall x4 all':
        's3_tall p0 part0 ; s3_tall p1 part0 ; s3_tall p2 part0 ; s3_tall p3 part0',
    's3 tall bf16':
        'k_gemm_skinny<64,16,0,false,true,0> g784,1,1 b512 l32768 i0 p0a1w0',
    'tall_ln':
        'k_ln_silu_rows<1> g960,1,1 b256 l0 p0 ; k_gemm_skinny<64,16,0,false,true,0> g784,1,1 b512 l32768 i0 p0a7w0',
    'tall_ln K1024 x2':
        'k_ln_silu_rows<4> g960,1,1 b256 l0 p0 ; k_ln_silu_rows<1> g960,1,1 b256 l0 p1 ; k_gemm_tile<64,64,32,false,false,true,4> g480,1,1 b256 l0 i1 i2 p0a7w0 p1a7w0',
    'tall_ln planes':
        'k_ln_silu_rows<1> g960,1,1 b256 l0 p0 ; s3_tall p0 part0',
    'tall_ln M1023':
        'k_gemm_skinny<64,16,1,false,true,0> g208,1,1 b512 l64000 i0 p0a1w0',
    'tall_ln no a_out':
        'k_gemm_skinny<64,16,1,false,true,0> g784,1,1 b512 l64000 i0 p0a1w0',
    'tall_ln K202':
        'k_gemm_skinny<64,16,1,false,false,0> g784,1,1 b512 l32768 i0 p0a1w0',
    'tall_ln K1028':
        'k_gemm_skinny<64,16,1,false,true,0> g784,1,1 b512 l32768 i0 p0a1w0',
    'tall_ln K0':
        'k_gemm_skinny<64,16,1,false,true,0> g784,1,1 b512 l32768 i0 p0a1w0',
    'tall_ln A2':
        'k_gemm_skinny<64,16,1,false,true,0> g784,1,1 b512 l64000 i0 p0a1w0',
    'tall_ln lda201':
        'k_gemm_skinny<64,16,1,false,false,0> g784,1,1 b512 l32768 i0 p0a1w0',
    'tall_ln A off':
        'k_gemm_skinny<64,16,1,false,false,0> g784,1,1 b512 l32768 i0 p0a1w0',
    'tall_ln gamma off':
        'k_gemm_skinny<64,16,1,false,true,0> g784,1,1 b512 l64000 i0 p0a1w0',
    'tall_ln beta off':
        'k_gemm_skinny<64,16,1,false,true,0> g784,1,1 b512 l64000 i0 p0a1w0',
    'tall_ln a_out off':
        'k_gemm_skinny<64,16,1,false,true,0> g784,1,1 b512 l64000 i0 p0a1w0',
    'tall_ln ld_aout 201':
        'k_gemm_skinny<64,16,1,false,true,0> g784,1,1 b512 l64000 i0 p0a1w0',
    'tall_ln epi':
        'k_gemm_skinny<16,16,1,false,true,2> g240,1,1 b512 l25600 i0 p0a1w0',
    'tall_ln rows 2^31 lda':
        'k_gemm<64,64,1,false,false> g240,1,1 b256 l0 p0a1w0',
    'tall_ln rows 2^31 ld_aout':
        'k_gemm<64,64,1,false,false> g240,1,1 b256 l0 p0a1w0',
    'tall_ln rows below 2^31':
        'k_ln_silu_rows<1> g960,1,1 b256 l0 p0 ; k_gemm<64,64,0,false,false> g240,1,1 b256 l0 p0a7w0',
    'tall_ln x2 one':
        'k_gemm_skinny<64,16,1,false,true,0> g992,1,1 b512 l64000 i2 p0a1w0 p1a1w0',
    'ln_sample':
        'k_ln_gemm_sample<13> g256,1,1 b256 l73472 p0a1w0',
    'ln_sample K256':
        'k_ln_gemm_sample<16> g8,1,1 b256 l88832 p0a1w0',
    'ln_sample C16':
        'k_gemm_skinny<16,32,1,false,true,1> g512,1,1 b512 l38400 i0 p0a1w0',
    'ln_sample K260':
        'k_gemm_skinny<16,32,1,false,true,1> g512,1,1 b512 l50688 i0 p0a1w0',
    'sample plain M65':
        'k_gemm_skinny<16,32,0,false,true,1> g160,1,1 b512 l16384 i0 p0a1w0',
    'actor':
        'k_gemm_skinny<16,16,1,false,true,2> g16,1,1 b512 l25600 i0 p0a1w0',
    'actor M1024':
        'k_gemm_skinny<16,16,1,false,true,2> g64,1,1 b512 l25600 i0 p0a1w0',
    'err count 0':
        'E 1001 gemm_launch: bad problem count 0',
    'err count 5':
        'E 1001 gemm_launch: bad problem count 5',
    'err negative':
        'E 1001 gemm_launch: negative dims',
    'err sampler C3':
        'E 1001 gemm_launch: sampler epilogue needs C | 32 and N == R*C (C=3 R=10 N=30)',
    'err actor N':
        'E 1001 gemm_launch: actor epilogue needs N == 2A <= 16',
    'err epi M4097':
        'E 1001 gemm_launch: fused epilogues need the NT skinny path',
    'err epi NN':
        'E 1001 gemm_launch: fused epilogues need the NT skinny path',
    'err lnbwd K1028':
        'E 1001 gemm_launch: AM_LNBWD needs K % 4 == 0, K <= 1024, 16-byte aligned rows (K=1028)',
    'err lnbwd K260 rows64':
        'E 1001 gemm_launch: AM_LNBWD needs K % 4 == 0, K <= 256, 16-byte aligned rows (K=260)',
    'err lnbwd pre off':
        'E 1001 gemm_launch: AM_LNBWD needs K % 4 == 0, K <= 1024, 16-byte aligned rows (K=200)',
    'err stebwd rows64':
        'E 1001 gemm_launch: AM_STEBWD needs 16-row tiles (gemm_bwd_rows16), K % C == 0, C/4 a power of two, K <= 256, 16-byte aligned rows (K=256 C=32)',
    'err stebwd C24':
        'E 1001 gemm_launch: AM_STEBWD needs 16-row tiles (gemm_bwd_rows16), K % C == 0, C/4 a power of two, K <= 1024, 16-byte aligned rows (K=240 C=24)',
    'err lnbwd offsets':
        'E 1001 gemm: LayerNorm-backward prologue needs the staged NT skinny path',
    'err amode':
        'E 1001 gemm_launch: bad amode',
    'lnbwd K256 rows64':
        'k_gemm_skinny<64,16,4,false,true,0> g208,1,1 b512 l84480 i0 p0a1w0',
    'lnbwd K1024':
        'k_gemm_skinny<16,16,4,false,true,0> g208,1,1 b512 l132096 i0 p0a1w0',
    'nn skinny':
        'k_gemm_skinny<16,16,0,true,true,0> g208,1,1 b512 l8192 i0 p0a1w0',
    'nn tile':
        'k_gemm_tile<64,64,32,false,true,true,4> g64,4,1 b256 l0 i4 i0 p0a1w1 ; k_splitk_finish g1024,1,1 b256 l0 i4 p0a1w1',
    'tn tile':
        'k_gemm_tile<64,64,32,true,true,true,4> g104,1,1 b256 l0 i1 i0 p0a1w0',
    'tn tile x4 ws':
        'k_gemm_tile<64,64,32,true,true,true,4> g64,4,1 b256 l0 i4 i4 p0a1w1 p1a1w1 p2a1w1 p3a1w1 ; k_splitk_finish g157,1,4 b256 l0 i4 p0a1w1 p1a1w1 p2a1w1 p3a1w1',
    'legacy nn below':
        'k_gemm<32,32,0,false,true> g256,1,1 b256 l0 p0a1w0',
    'legacy nn at':
        'k_gemm<64,64,0,false,true> g64,1,1 b256 l0 p0a1w0',
    'legacy tn below':
        'k_gemm<32,32,0,true,true> g256,1,1 b256 l0 p0a1w0',
    'legacy tn at':
        'k_gemm<64,64,0,true,true> g64,1,1 b256 l0 p0a1w0',
    'legacy conv below':
        'k_gemm<32,32,2,false,false> g256,1,1 b256 l0 p0a1w0',
    'legacy conv at':
        'k_gemm<64,64,2,false,false> g64,1,1 b256 l0 p0a1w0',
    'legacy conv_src below':
        'k_gemm<32,32,3,false,false> g256,1,1 b256 l0 p0a1w0',
    'legacy conv_src at':
        'k_gemm<64,64,3,false,false> g64,1,1 b256 l0 p0a1w0',
    'legacy x2 at':
        'k_gemm<64,64,2,false,false> g32,1,2 b256 l0 p0a1w0 p1a1w0',
    'offsets below':
        'k_gemm_skinny<64,16,0,false,true,0> g256,1,1 b512 l32768 i0 p0a1w0',
    'offsets at':
        'k_gemm<64,64,0,false,false> g64,1,1 b256 l0 p0a1w0',
    'offsets W at':
        'k_gemm<64,64,0,false,false> g64,1,1 b256 l0 p0a1w0',
    'offsets tile below':
        'k_gemm_tile<64,64,64,false,false,true,8> g256,1,1 b512 l0 i1 i0 p0a1w0',
    'offsets tile at':
        'k_gemm_skinny<64,16,0,false,true,0> g1024,1,1 b512 l32768 i0 p0a1w0',
}


def test_cases_and_table_cover_each_other():
    assert sorted(_cases()) == sorted(EXPECT)


@pytest.mark.parametrize("name", sorted(EXPECT))
def test_route_is_the_recorded_one(name):
    lay, amode, probs = _cases()[name]
    assert route(lay, amode, probs) == EXPECT[name]


def test_required_routes():
    """The routes the update phase at B = 256 / 512 leans on."""
    r = lambda n: route(*_cases()[n])
    assert r("lnbwd B256 N600 K200").startswith("k_gemm_skinny<16,48,4,false,true,0> g208,1,1 ")
    assert r("stebwd B512 N200 K1024").startswith("k_gemm_skinny<16,16,5,false,true,0> g416,1,1 ")


# ---------------------------------------------------------------------------
# the shared tile predicates against the hand copies they replace
# ---------------------------------------------------------------------------
SK_LN_MAXF, DR_SKW = 33280, 8


def _kpad(K):
    return K + ((8 - (K & 15)) & 15)


def old_staged(amode, mt, nt, K):
    """k_gemm_skinny's `staged` before the shared predicate (VEC, NT)."""
    sv = 4 if (mt == 16 and nt <= 32) else 1
    return amode in (LNSILU, LNBWD, STEBWD) and K // 4 <= 64 * sv and (mt + nt) * _kpad(K) <= SK_LN_MAXF


def old_skinny_lds_floats(amode, mt, nt, K):
    """skinny_lds_floats before the shared predicate (vec, NT, one problem)."""
    red = DR_SKW * (mt // 16) * (nt // 16) * 4 * 64
    if old_staged(amode, mt, nt, K):
        return max(red, (mt + nt) * _kpad(K))
    if amode == LNSILU and mt * _kpad(K) <= SK_LN_MAXF and K // 4 <= 64 * (8 if mt == 16 else 2):
        return max(red, mt * _kpad(K))
    return red


# (amode, MT, NT) -> the smallest problem shape that lands on that tile
TILE_SHAPES = {
    (LNSILU, 16, 16): dict(M=16, N=16), (LNSILU, 16, 32): dict(M=64, N=1040), (LNSILU, 64, 16): dict(M=4096, N=256),
    (LNSILU, 64, 32): dict(M=4096, N=128, epi=SAMPLE, C=16, R=8), (LNSILU, 16, 32, "s"): dict(M=16, N=32, epi=SAMPLE, C=16, R=2),
    (LNBWD, 16, 16): dict(M=16, N=16), (LNBWD, 16, 32): dict(M=64, N=4096), (LNBWD, 16, 48): dict(M=64, N=2080),
    (LNBWD, 64, 16): dict(M=4096, N=256), (STEBWD, 16, 16): dict(M=16, N=16), (STEBWD, 16, 32): dict(M=64, N=1040),
}


def sweep_prob(key, K):
    amode, kw = key[0], TILE_SHAPES[key]
    fl = {LNSILU: LN, LNBWD: LN | PRE | AOUT, STEBWD: PRE}[amode]
    return prob(kw["M"], kw["N"], K, fl, epi=kw.get("epi", 0), C=kw.get("C", 4 if amode == STEBWD else 0), R=kw.get("R", 0))


def sweep_sha(key, route_fn):
    """sha256 over the routes (tile, grid, LDS bytes, or the error) of K = 4 ... 2100 on one tile shape."""
    import hashlib
    return hashlib.sha256("\n".join(route_fn(G_NT, key[0], [sweep_prob(key, K)]) for K in range(4, 2101, 4)).encode()).hexdigest()[:16]


# the parent's side of the sweep: sweep_sha of its recorded launches (its skinny_lds_floats sized their LDS)
SWEEP_PARENT = {
    '(1, 16, 16)': '10786455cd2e3ad7',
    '(1, 16, 32)': '22084a6d13bd40a0',
    "(1, 16, 32, 's')": 'd926c7c4c7d29692',
    '(1, 64, 16)': 'f9da8f53cda44c00',
    '(1, 64, 32)': 'b93bcafde639332b',
    '(4, 16, 16)': '8c8c5ca27cbade9f',
    '(4, 16, 32)': 'fab8892884951108',
    '(4, 16, 48)': 'c42a8d7b82baf54f',
    '(4, 64, 16)': 'c9b9dd3a0c0d4a50',
    '(5, 16, 16)': '71b68a473a99ef2b',
    '(5, 16, 32)': '7f29e249dfefddee',
}


@pytest.mark.parametrize("key", sorted(TILE_SHAPES, key=str))
def test_sweep_equals_the_recorded_parent(key):
    assert sweep_sha(key, route) == SWEEP_PARENT[str(key)]


@pytest.mark.parametrize("key", sorted(TILE_SHAPES, key=str))
def test_shared_predicate_matches_the_old_copies(key):
    """The same sweep against the old formulas written out, so that a mismatch names its K."""
    amode, mt, nt = key[:3]
    for K in range(4, 2101, 4):
        p = sweep_prob(key, K)
        steps, err = plan_steps(G_NT, amode, [p])
        if amode == LNSILU:
            assert err is None and len(steps) == 1, (K, err)
        if err is not None:  # a backward prologue the planner refuses: never one the widest fallback tile could stage
            assert err[0] == DR_E_INVALID and not old_staged(amode, mt, 16, K), (K, err)
            continue
        s = steps[0]
        assert s[0] == F_SKINNY
        bm, bn, lds = s[1], s[2], s[17]
        if amode == LNSILU:
            assert (bm, bn) == (mt, nt), (K, bm, bn)
        else:  # the planner narrows a backward tile that cannot stage K; what it picks is staged
            assert bm == mt and bn in (16, 32, 48) and bn <= nt, (K, bm, bn)
            assert old_staged(amode, bm, bn, K), (K, bm, bn)
            if K == 64:  # the shape does land on the tile it is listed under
                assert bn == nt, (bm, bn)
        assert lds == 4 * old_skinny_lds_floats(amode, bm, bn, K), (K, bm, bn, lds)


# ---------------------------------------------------------------------------
# gemm_bwd_fusable (the planner takes the problem on k_gemm_skinny) against the
# three conditions it replaced, at the shapes the engine asks about
# ---------------------------------------------------------------------------
def old_rows16(M, N):
    t16 = -(-M // 16) * -(-N // 16)
    return M <= 64 or (M <= 4096 and t16 <= 640)


def fusable_rows(amode, p):
    steps, err = plan_steps(G_NT, amode, [p])
    return steps[0][1] if (err is None and len(steps) == 1 and steps[0][0] == F_SKINNY) else 0


@pytest.mark.parametrize("B", [16, 64, 65, 128, 256, 512, 4096])
def test_fused_backward_admission(B):
    for hd, lat, h, a, cols in ((600, 1024, 200, 200, 32), (64, 64, 32, 32, 8)):  # FULL, SMALL
        # lnbwd_nt (engine_util.h): prior and actor layers, N = their input width
        for N, K in ((h, h), (hd, h), (a, a), (hd + lat, a)):
            r16 = old_rows16(B, N)
            old_ok = K % 4 == 0 and K <= (1024 if r16 else 256) and B <= 4096
            rows = fusable_rows(LNBWD, prob(B, N, K, LN | PRE | AOUT | ACC))
            assert bool(rows) == old_ok, (B, N, K)
            assert (rows == 16) == (old_ok and r16), (B, N, K)
        # the prior head's softmax-STE backward (engine.hip imagine_bwd)
        gl = cols // 4
        old_ok = lat <= 1024 and cols % 4 == 0 and gl <= 64 and gl & (gl - 1) == 0 and old_rows16(B, h)
        assert bool(fusable_rows(STEBWD, prob(B, h, lat, PRE, C=cols))) == old_ok, (B, lat, cols)
