// 1x1 convolution (stride 1) as a streaming GEMM (included by conv_core.hip).
//
// The generic implicit-GEMM kernel pays for a halo tile, virtual rows and per-slot index math that a
// 1x1 conv does not need, and it stages K in 64-byte (32-channel) chunks -- one barrier pair per 8
// MFMAs per wave, 8 pipeline stages per tile for Ci = 256.  Here:
//   * pixels are a flat range [0, B*H*W): tile t = pixels [256 t, 256 t + 256), all addresses are
//     pixel * C + channel (no divisions, no image-boundary loops);
//   * K is staged G 64-byte sub-chunks at a time (G = 2: 64 channels, G = 4: 128 channels bf16), the
//     "tap" loop of the 3x3 kernel becomes a loop over the G sub-chunks of one pixel row, so a stage
//     carries G x 8 MFMAs per wave per barrier pair and Ci = 256 is 2 stages;
//   * LDS rows are G*64 + 32 bytes (odd multiple of 32 B: conflict-free ds_read_b128), filters
//     [co][G*64+32] are the plain [Co][Ci] weight rows.
// Block = 8 waves (4 pixel x 2 channel), 256 pixels x 64 output channels, 4 x 2 accumulator tiles per
// wave, operands swapped like conv_core_kernel (filters = MFMA A, pixels = B) and the same fused
// epilogue (epilogue_tile: bias, addend, mask_y / mask_z, statistics) and statistics flush.
// ZM (round 5): the source is a residual block end z = ReLU(BN(x) + y) formed on load (STL_SRC_BNADD; Q = true: two tensors);
// every (pixel, channel) of z is staged exactly once per channel block, so channel block 0 also writes it to p.src_out -- the
// first 1x1 convolution of the next layer1 unit absorbs the unit's sum launch (a 113 MB read-modify-write pass each).
template <typename T, int G, bool Q, int OCC, typename TY = T, int EO = -1, bool ZM = false>
__global__ __launch_bounds__(512, OCC) void conv1x1_kernel(const ConvK k) {  // OCC 4: 128 VGPRs -> two blocks per CU
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NTHR = 512, WM = 4, MT = 4, NTW = 2, BCO = 64, TPX = 256;
    constexpr int KV = ET<T>::KV, CK = ET<T>::CK;
    constexpr int PSG = G * 64 + 32;         // LDS bytes per pixel row / per filter row
    constexpr int VPP = 4 * G;               // 16-byte vectors per row and stage
    constexpr int RPT = NTHR / VPP;          // rows covered by one pass of the block
    constexpr int NVA = TPX / RPT;           // staging vectors per thread (pixels)
    constexpr int NVB = BCO / RPT;           // staging vectors per thread (filters)
    constexpr int GK = G * CK;               // channels per stage
    static_assert(NVB >= 1, "filter staging needs at least one vector per thread");
    const stl_conv& p = k.p;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, g = lane >> 4;
    const int wm = wave % WM, wn = wave / WM;
    const int bl = blockIdx.x >> 3;          // channel blocks of a pixel tile are neighbours on one XCD
    const int by = bl % k.ny, lx = bl / k.ny;
    const int n0 = by * BCO;
    const int xcd = blockIdx.x & 7, nx = (gridDim.x >> 3) / k.ny;
    const int P = p.B * p.Ho * p.Wo;

    float* cs = reinterpret_cast<float*>(smem + k.off_cs);  // [3][cipad] source transform
    float* cm = reinterpret_cast<float*>(smem + k.off_cm);  // [4][BCO]   mask BN: a, b, mean, rstd
    char* sA = smem + k.off_a;
    char* sB = smem + k.off_b;

    for (int c = tid; c < k.cipad; c += NTHR) {
        float a = 0.f, b = 0.f, cc = 0.f;
        if (c < p.Ci) src_consts(p.src, c, p.Ci, a, b, cc);
        cs[c] = a, cs[k.cipad + c] = b, cs[2 * k.cipad + c] = cc;
    }
    if (p.mask_y) {
        for (int c = tid; c < BCO; c += NTHR) {
            float a = 0.f, b = 0.f, mu = 0.f, rs = 0.f;
            if (n0 + c < p.Co) {
                bn_mean_rstd(p.mask_bn, n0 + c, p.Co, mu, rs);
                bn_affine(p.mask_bn.gamma[n0 + c], p.mask_bn.beta[n0 + c], mu, rs, a, b);
            }
            cm[c] = a, cm[BCO + c] = b, cm[2 * BCO + c] = mu, cm[3 * BCO + c] = rs;
        }
    }

    const int a_part = tid % VPP, a_row = tid / VPP;   // this thread's 16-byte column and first row
    V16 ra[NVA], rq[Q ? NVA : 1], rb[NVB];

    // unconditional loads, clamped addresses (see conv_core_kernel)
    auto issue = [&](int P0, int k0, bool en) {
        const int ch = k0 + a_part * KV;
        const bool chok = en && ch < p.Ci;
#pragma unroll
        for (int i = 0; i < NVA; ++i) {
            const int pix = P0 + a_row + i * RPT;
            const size_t off = (chok && pix < P) ? (size_t)pix * p.Ci + ch : 0;
            ra[i] = ldg16((const char*)p.src.x + off * sizeof(T));
            if (Q) rq[i] = ldg16((const char*)p.src.y + off * sizeof(T));
        }
        if (!k.wres) {
#pragma unroll
            for (int i = 0; i < NVB; ++i) {
                const int n = n0 + a_row + i * RPT;
                const size_t off = (chok && n < p.Co) ? (size_t)n * p.Ci + ch : 0;
                rb[i] = ldg16((const char*)p.w + off * sizeof(T));
            }
        }
    };
    const float relu_lo = p.src.relu ? 0.f : -INFINITY;
    auto write_lds = [&](int P0, int k0) {
        const int ch = k0 + a_part * KV;
        const bool chok = ch < p.Ci;
        const int chc = chok ? ch : 0;
#pragma unroll
        for (int i = 0; i < NVA; ++i) {
            const bool ok = chok && (P0 + a_row + i * RPT) < P;
            V16 val = ra[i];
            if constexpr (ZM) {
                val = xform_bnadd<T>(val, rq[i], cs + chc, cs + k.cipad + chc, relu_lo);
                if (ok && by == 0 && p.src_out) stg16((char*)p.src_out + ((size_t)(P0 + a_row + i * RPT) * p.Ci + ch) * sizeof(T), val);
            } else if (Q)
                val = xform_bnbwd<T, TY>(val, rq[i], cs + chc, cs + k.cipad + chc, cs + 2 * k.cipad + chc);
            else if (p.src.mode != STL_SRC_PLAIN)
                val = xform_bn<T>(val, cs + chc, cs + k.cipad + chc, relu_lo);
            mask16(val, ok);
            *reinterpret_cast<V16*>(sA + (a_row + i * RPT) * PSG + a_part * 16) = val;
        }
        if (!k.wres) {
#pragma unroll
            for (int i = 0; i < NVB; ++i) {
                V16 val = rb[i];
                mask16(val, chok && (n0 + a_row + i * RPT) < p.Co);
                *reinterpret_cast<V16*>(sB + (a_row + i * RPT) * PSG + a_part * 16) = val;
            }
        }
    };

    if (k.wres) {  // the whole K fits one stage: filters stay resident in LDS for all tiles
        const bool chok = a_part * KV < p.Ci;
#pragma unroll
        for (int i = 0; i < NVB; ++i) {
            const int n = n0 + a_row + i * RPT;
            const size_t off = (chok && n < p.Co) ? (size_t)n * p.Ci + a_part * KV : 0;
            rb[i] = ldg16((const char*)p.w + off * sizeof(T));
        }
    }

    f2v s0[NTW][2], s1[NTW][2];
#pragma unroll
    for (int ni = 0; ni < NTW; ++ni)
#pragma unroll
        for (int h = 0; h < 2; ++h) s0[ni][h] = f2v{0.f, 0.f}, s1[ni][h] = f2v{0.f, 0.f};
    f32x4 acc[MT][NTW];
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
        for (int ni = 0; ni < NTW; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

    int xoff[MT];
#pragma unroll
    for (int mi = 0; mi < MT; ++mi) xoff[mi] = ((wm * MT + mi) * 16 + r16) * PSG + g * 16;
    const int woff = (wn * NTW * 16 + r16) * PSG + g * 16;

    const int T8 = (k.npt + 7) >> 3;
    int it = lx, t = xcd * T8 + it, ch0 = 0;
    bool have = (it < T8) && (t < k.npt);
    issue(t * TPX, 0, have);
    if (k.wres) {
        const bool chok = a_part * KV < p.Ci;
#pragma unroll
        for (int i = 0; i < NVB; ++i) {
            V16 val = rb[i];
            mask16(val, chok && (n0 + a_row + i * RPT) < p.Co);
            *reinterpret_cast<V16*>(sB + (a_row + i * RPT) * PSG + a_part * 16) = val;
        }
    }
    __syncthreads();  // constants + resident filters visible

    while (have) {
        const int P0 = t * TPX;
        write_lds(P0, ch0 * GK);
        __syncthreads();
        const bool last_chunk = (ch0 + 1 == k.nchunks);
        int itn = it, tn = t, chn = ch0 + 1;
        bool have_n = true;
        if (last_chunk) {
            itn = it + nx, tn = xcd * T8 + itn, chn = 0;
            have_n = (itn < T8) && (tn < k.npt);
        }
        issue(tn * TPX, chn * GK, have_n);  // next stage's loads land during the MFMAs below
#pragma unroll
        for (int sub = 0; sub < G; ++sub) {
            V16 wf[NTW], xf[MT];
#pragma unroll
            for (int ni = 0; ni < NTW; ++ni) wf[ni] = *reinterpret_cast<const V16*>(sB + woff + ni * 16 * PSG + sub * 64);
#pragma unroll
            for (int mi = 0; mi < MT; ++mi) xf[mi] = *reinterpret_cast<const V16*>(sA + xoff[mi] + sub * 64);
#pragma unroll
            for (int mi = 0; mi < MT; ++mi)
#pragma unroll
                for (int ni = 0; ni < NTW; ++ni) mma16<T>(acc[mi][ni], wf[ni], xf[mi]);
        }
        __syncthreads();  // everyone is done with sA / sB of this stage
        if (last_chunk) {
#pragma unroll
            for (int mi = 0; mi < MT; ++mi) {
                const int pix = P0 + (wm * MT + mi) * 16 + r16;
                const bool pok = pix < P;
                epilogue_tile<T, NTW, BCO, false, TY, EO>(p, acc[mi], cm, pok, pok ? (size_t)pix * p.Co : 0, n0, wn * NTW * 16, g, s0, s1);
            }
        }
        it = itn, t = tn, ch0 = chn, have = have_n;
    }
    // ---- statistics flush (as conv_core_kernel)
    double* dst = p.out_stats ? p.out_stats : p.red;
    if (dst) {
        xor_reduce_stats<NTW>(s0, s1);
        float* red = reinterpret_cast<float*>(smem + k.off_red);  // [WM][2][BCO]
        __syncthreads();
        if (r16 == 0) {
#pragma unroll
            for (int ni = 0; ni < NTW; ++ni)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int cl = (wn * NTW + ni) * 16 + 4 * g + r;
                    red[(wm * 2 + 0) * BCO + cl] = s0[ni][r >> 1][r & 1];
                    red[(wm * 2 + 1) * BCO + cl] = s1[ni][r >> 1][r & 1];
                }
        }
        __syncthreads();
        for (int e = tid; e < 2 * BCO; e += NTHR) {
            const int which = e / BCO, cl = e - which * BCO;
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < WM; ++w) s += red[(w * 2 + which) * BCO + cl];
            if (n0 + cl < p.Co)
                atomicAdd(dst + (size_t)(blockIdx.x & (STL_NSHARD - 1)) * 2 * p.Co + which * p.Co + n0 + cl, (double)s);
        }
    }
}

template <typename T, typename TY, int G, bool Q, int OCC, int EO = -1, bool ZM = false>
int launch_1x1(const ConvK& k, dim3 grid, size_t lds, hipStream_t st) {
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv1x1_kernel<T, G, Q, OCC, TY, EO, ZM>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  160 * 1024);
        attr_done = true;
    }
    STL_LAUNCH((conv1x1_kernel<T, G, Q, OCC, TY, EO, ZM>), grid, dim3(512), lds, st, k);
    static char nbuf[160];
    static const char* nm = stl_kname<T>(nbuf, "conv1x1_kernel", {G, Q, OCC, stl_code<TY>(), EO, ZM});
    stl_note_kernel(nm, true);
    STL_LAUNCH_CHECK("conv1x1");
    return 0;
}

// 1x1, stride 1, both channel counts >= 64: the streaming kernel
static bool use_1x1(const stl_conv& p) { return p.ks == 1 && p.stride == 1 && !p.stuff && p.Ci >= 64 && p.Co >= 64; }

template <typename T, typename TY>
int run_1x1(const stl_conv& p, hipStream_t st) {
    constexpr int CK = ET<T>::CK;
    // G = 2 (64 channels bf16 per stage, 51 KB of LDS, three blocks per CU) measured faster than G = 4
    // (one block per CU) for every 1x1 layer of the network: 64->256 68 vs 91 us, 256->64 45 vs 60 us
    constexpr int G = 2;
    const int gk = G * CK, psg = G * 64 + 32;
    ConvK k;
    memset(&k, 0, sizeof(k));
    k.p = p;
    k.nchunks = ceil_div(p.Ci, gk);
    k.cipad = k.nchunks * gk;
    k.wres = k.nchunks == 1;
    int off = 3 * k.cipad * 4;
    k.off_cs = 0, k.off_cm = off;
    off += 4 * 64 * 4;
    off = (off + 15) & ~15;
    k.off_a = off;
    off += 256 * psg;
    k.off_b = off;
    off += 64 * psg;
    k.off_red = k.off_a;  // reused after the last stage
    const size_t lds = (size_t)off;
    const int P = p.B * p.Ho * p.Wo;
    k.npt = ceil_div(P, 256);
    k.ny = ceil_div(p.Co, 64);
    int gx = ceil_div(k.npt, 8) * 8;
    int cap = std::max(8, (512 / k.ny + 7) / 8 * 8);   // 512 blocks in total: two resident 8-wave blocks per CU (measured)
    if (const char* e = getenv("STL_CONV_GRID_CAP")) cap = atoi(e) > 0 ? (atoi(e) + 7) / 8 * 8 : cap;
    if (gx > cap) gx = cap;
    dim3 grid(gx * k.ny, 1);
    if (getenv("STL_CONV_DEBUG"))
        fprintf(stderr, "[stl conv1x1] %dx%d Ci%d Co%d: G=%d npt=%d grid=(%d x %d) lds=%zu nchunks=%d\n", p.Ho, p.Wo, p.Ci, p.Co, G, k.npt, gx,
                k.ny, lds, k.nchunks);
    if (p.src.mode == STL_SRC_BNADD) {   // block-end source: forward convolutions only (plain epilogue)
        if constexpr (std::is_same<T, TY>::value) {
            const int eoz = epi_code(p);
            if (eoz == 8) return launch_1x1<T, T, 2, true, 4, 8, true>(k, grid, lds, st);
            if (eoz == 0) return launch_1x1<T, T, 2, true, 4, 0, true>(k, grid, lds, st);
        }
        return stl_set_error("conv1x1: a BNADD source takes no epilogue operands");
    }
    const bool q = p.src.mode == STL_SRC_BNBWD;
    // the data-gradient form keeps its 128-VGPR budget (31 spilled registers): two blocks per CU measured faster end to end
    // than the spill-free build at one block (20.36 vs 20.49 ms per step in round 1)
    const char* noeo = getenv("STL_CONV_NO_EO");
    const int eo = (noeo && (atoi(noeo) & 2)) ? -1 : epi_code(p);   // compile-time epilogue operand set where the planner's forms match
    if (q) {
        if constexpr (!stl_fwd_only<T>) {
            // (the mask_y forms, EO 1 / 7, spill 35 - 50 registers at this kernel's 128-register budget: 14.21 vs 14.06 ms per step)
            if (eo == 2) return launch_1x1<T, TY, 2, true, 4, 2>(k, grid, lds, st);
            return launch_1x1<T, TY, 2, true, 4>(k, grid, lds, st);
        }
    }
    if constexpr (std::is_same<T, TY>::value) {
        if (eo == 8) return launch_1x1<T, T, 2, false, 4, 8>(k, grid, lds, st);
        return launch_1x1<T, T, 2, false, 4>(k, grid, lds, st);
    }
    return stl_set_error("conv1x1: no kernel for this dtype combination");
}
