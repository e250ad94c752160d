// Shared device helpers of the conv kernels: packed-math "normalise on load" transforms and the
// fused epilogue of one 16-pixel tile (all of a wave's channel tiles), written so that hipcc emits
// v_pk_fma_f32 / v_cvt_pk_bf16_f32 and no per-element branches.
typedef __attribute__((ext_vector_type(2))) float f2v;
// a * b + c with ONE rounding, written out: left to the compiler, the contraction of `a * b + c` differs between instantiations
// of the same source (v_pk_fma_f32 in one, v_pk_mul_f32 + v_pk_add_f32 in another), and two kernels that should agree bit for bit
// differ by an ulp of the 16-bit result in a few elements per million (round 5: conv_r2_kernel against conv_core_kernel, mixed mode)
__device__ __forceinline__ f2v fma2(f2v a, f2v b, f2v c) { return __builtin_elementwise_fma(a, b, c); }

// 16-byte vector of TS elements -> KV packed pairs of floats (KV = 8: four pairs per vector; fp32: two pairs)
template <typename TS>
__device__ __forceinline__ void unpack_pairs(const V16& x, f2v* v) {
    if constexpr (sizeof(TS) == 2) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float lo, hi;
            unpack2<TS>(x.w[i], lo, hi);
            v[i][0] = lo, v[i][1] = hi;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 2; ++i) v[i][0] = __uint_as_float(x.w[2 * i]), v[i][1] = __uint_as_float(x.w[2 * i + 1]);
    }
}
template <typename TO>
__device__ __forceinline__ V16 pack_pairs(const f2v* u) {
    V16 o;
    if constexpr (sizeof(TO) == 2) {
#pragma unroll
        for (int i = 0; i < 4; ++i) o.w[i] = pack2<TO>(u[i][0], u[i][1]);
    } else {
#pragma unroll
        for (int i = 0; i < 2; ++i) o.w[2 * i] = __float_as_uint(u[i][0]), o.w[2 * i + 1] = __float_as_uint(u[i][1]);
    }
    return o;
}

// v = max(a*x + b, lo)  per channel; a/b = LDS pointers to this vector's KV channel constants
// (lo = 0 for ReLU, -inf for none).  16-byte aligned.  TS: stored type of x, T: type of the result (the MFMA operand) --
// they differ only in the weight gradient of the mixed mode (h is read as f16 and multiplied as bf16).
template <typename T, typename TS = T>
__device__ __forceinline__ V16 xform_bn(const V16& x, const float* ca, const float* cb, float lo) {
    static_assert(sizeof(T) == sizeof(TS), "source and operand types must have the same width");
    constexpr int NP = sizeof(T) == 2 ? 4 : 2;
    const f2v* a2 = reinterpret_cast<const f2v*>(ca);
    const f2v* b2 = reinterpret_cast<const f2v*>(cb);
    f2v v[NP], u[NP];
    unpack_pairs<TS>(x, v);
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const f2v t = fma2(a2[i], v[i], b2[i]);
        u[i][0] = max_lo<T>(t[0], lo), u[i][1] = max_lo<T>(t[1], lo);
    }
    return pack_pairs<T>(u);
}
// plain source stored as TS, multiplied as T (weight gradient of the mixed mode: f16 sum -> bf16 operand)
template <typename T, typename TS>
__device__ __forceinline__ V16 xform_cvt(const V16& x) {
    if constexpr (std::is_same<T, TS>::value) {
        return x;
    } else {
        f2v v[4];
        unpack_pairs<TS>(x, v);
        return pack_pairs<T>(v);
    }
}

// residual block end on load: v = max(a*x + b + y, lo) per channel (x = raw conv output, y = skip tensor)
template <typename T>
__device__ __forceinline__ V16 xform_bnadd(const V16& x, const V16& y, const float* ca, const float* cb, float lo) {
    constexpr int NP = sizeof(T) == 2 ? 4 : 2;
    const f2v* a2 = reinterpret_cast<const f2v*>(ca);
    const f2v* b2 = reinterpret_cast<const f2v*>(cb);
    f2v v[NP], q[NP], u[NP];
    unpack_pairs<T>(x, v);
    unpack_pairs<T>(y, q);
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const f2v t = fma2(a2[i], v[i], b2[i]) + q[i];   // same association as the stand-alone sum kernel: BN term first, then the skip
        u[i][0] = max_lo<T>(t[0], lo), u[i][1] = max_lo<T>(t[1], lo);
    }
    return pack_pairs<T>(u);
}

// BatchNorm backward on load: v = a*dt + b*y + c per channel (dt stored as T, y -- a FORWARD tensor -- as TY)
template <typename T, typename TY = T>
__device__ __forceinline__ V16 xform_bnbwd(const V16& dt, const V16& y, const float* ca, const float* cb, const float* cc) {
    static_assert(sizeof(T) == sizeof(TY), "gradient and forward types must have the same width");
    constexpr int NP = sizeof(T) == 2 ? 4 : 2;
    const f2v* a2 = reinterpret_cast<const f2v*>(ca);
    const f2v* b2 = reinterpret_cast<const f2v*>(cb);
    const f2v* c2 = reinterpret_cast<const f2v*>(cc);
    f2v d[NP], q[NP], u[NP];
    unpack_pairs<T>(dt, d);
    unpack_pairs<TY>(y, q);
#pragma unroll
    for (int i = 0; i < NP; ++i) u[i] = fma2(a2[i], d[i], fma2(b2[i], q[i], c2[i]));
    return pack_pairs<T>(u);
}

// The same transforms with the channel constants already in registers (kc: a / b / c as packed pairs): the two-image conv
// block reads them from LDS once per stage instead of once per staging vector (each read is followed by a full LDS wait).
template <typename T>
__device__ __forceinline__ V16 xform_bn_r(const V16& x, const f2v* a2, const f2v* b2, float lo) {
    constexpr int NP = sizeof(T) == 2 ? 4 : 2;
    f2v v[NP], u[NP];
    unpack_pairs<T>(x, v);
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const f2v t = fma2(a2[i], v[i], b2[i]);
        u[i][0] = max_lo<T>(t[0], lo), u[i][1] = max_lo<T>(t[1], lo);
    }
    return pack_pairs<T>(u);
}
template <typename T, typename TY = T>
__device__ __forceinline__ V16 xform_bnbwd_r(const V16& dt, const V16& y, const f2v* a2, const f2v* b2, const f2v* c2) {
    constexpr int NP = sizeof(T) == 2 ? 4 : 2;
    f2v d[NP], q[NP], u[NP];
    unpack_pairs<T>(dt, d);
    unpack_pairs<TY>(y, q);
#pragma unroll
    for (int i = 0; i < NP; ++i) u[i] = fma2(a2[i], d[i], fma2(b2[i], q[i], c2[i]));
    return pack_pairs<T>(u);
}

__device__ __forceinline__ void mask16(V16& v, bool ok) {
    const uint32_t keep = ok ? 0xFFFFFFFFu : 0u;
    v.w[0] &= keep, v.w[1] &= keep, v.w[2] &= keep, v.w[3] &= keep;
}

// 4 consecutive channels of one pixel as two packed pairs
template <typename T>
__device__ __forceinline__ void load4p(const void* base, size_t elem, f2v& lo, f2v& hi) {
    if constexpr (sizeof(T) == 2) {
        const uint2 v = *reinterpret_cast<const uint2*>((const char*)base + elem * 2);
        float a, b;
        unpack2<T>(v.x, a, b), lo[0] = a, lo[1] = b;
        unpack2<T>(v.y, a, b), hi[0] = a, hi[1] = b;
    } else {
        const V16 v = ldg16((const char*)base + elem * 4);
        lo[0] = __uint_as_float(v.w[0]), lo[1] = __uint_as_float(v.w[1]);
        hi[0] = __uint_as_float(v.w[2]), hi[1] = __uint_as_float(v.w[3]);
    }
}

// bf16, two neighbouring channel tiles at once: every lane loads the 16 contiguous bytes it also
// stores (8 channels of tile ni + (g & 1)), then v_permlane16_swap (its own inverse) hands each
// lane the 4 channels of BOTH tiles that the MFMA accumulator layout gives it.  One 16-byte load
// per tile pair instead of two 8-byte ones: 64 contiguous bytes per pixel and instruction.
// The load itself is issued early and kept raw (epilogue_fetch); this is the unpacking.
template <typename TE>
__device__ __forceinline__ void unpack4p_pair(const V16& v, f2v (&a)[2], f2v (&b)[2]) {
    const auto r0 = __builtin_amdgcn_permlane16_swap(v.w[0], v.w[2], false, false);
    const auto r1 = __builtin_amdgcn_permlane16_swap(v.w[1], v.w[3], false, false);
    const uint32_t a0 = r0[0], b0 = r0[1], a1 = r1[0], b1 = r1[1];
    float lo, hi;
    unpack2<TE>(a0, lo, hi), a[0][0] = lo, a[0][1] = hi;
    unpack2<TE>(a1, lo, hi), a[1][0] = lo, a[1][1] = hi;
    unpack2<TE>(b0, lo, hi), b[0][0] = lo, b[0][1] = hi;
    unpack2<TE>(b1, lo, hi), b[1][0] = lo, b[1][1] = hi;
}
template <typename T>
__device__ __forceinline__ void unpack4p(const V16& v, f2v& lo, f2v& hi) {
    if constexpr (sizeof(T) == 2) {
        float a, b;
        unpack2<T>(v.w[0], a, b), lo[0] = a, lo[1] = b;
        unpack2<T>(v.w[1], a, b), hi[0] = a, hi[1] = b;
    } else {
        lo[0] = __uint_as_float(v.w[0]), lo[1] = __uint_as_float(v.w[1]);
        hi[0] = __uint_as_float(v.w[2]), hi[1] = __uint_as_float(v.w[3]);
    }
}

// EO: which epilogue operands a launch has, as a compile-time set -- bit 0 mask_y (+ red), bit 1 addend, bit 2 mask_z,
// bit 3 out_stats, bit 4 bias, bit 5 output ReLU -- or -1: decided at run time from the pointers (epi_code() below maps a launch).  The run-time form costs ~25
// uniform branches per 16-pixel tile (a quarter of the epilogue's 3 us in the C >= 64 data gradient, round 4) and keeps the
// compiler from interleaving the tiles; the planner's two frequent sets (conv2 of a unit: mask_y; conv1 behind a block end:
// all three) get their own instantiations.
template <int EO> struct EpiOps {
    static __device__ __forceinline__ bool my(const stl_conv& p) { return EO >= 0 ? (EO & 1) != 0 : p.mask_y != nullptr; }
    static __device__ __forceinline__ bool ad(const stl_conv& p) { return EO >= 0 ? (EO & 2) != 0 : p.addend != nullptr; }
    static __device__ __forceinline__ bool mz(const stl_conv& p) { return EO >= 0 ? (EO & 4) != 0 : p.mask_z != nullptr; }
    static __device__ __forceinline__ bool bias(const stl_conv& p) { return EO >= 0 ? (EO & 16) != 0 : p.bias != nullptr; }
    static __device__ __forceinline__ bool orelu(const stl_conv& p) { return EO >= 0 ? (EO & 32) != 0 : p.out_relu != 0; }
    static __device__ __forceinline__ bool ostats(const stl_conv& p) { return EO >= 0 ? (EO & 8) != 0 : p.out_stats != nullptr; }
    static __device__ __forceinline__ bool red(const stl_conv& p) { return EO >= 0 ? (EO & 1) != 0 : p.red != nullptr; }
};

// The EO code of a launch if its operand set is one the kernels are specialised for, else -1 (host side).
// 8: forward conv with statistics; 1 / 7 / 2 / 0: the data-gradient forms of the planner (engine.py: conv2 of a unit, conv1 behind
// a fused block end, contributions to an exchange sum); 48: bias + ReLU, no statistics (the VGG feature extractors).
[[maybe_unused]] static inline int epi_code(const stl_conv& p) {
    if ((p.red != nullptr) != (p.mask_y != nullptr)) return -1;
    const int eo = (p.mask_y ? 1 : 0) | (p.addend ? 2 : 0) | (p.mask_z ? 4 : 0) | (p.out_stats ? 8 : 0) | (p.bias ? 16 : 0) | (p.out_relu ? 32 : 0);
    return (eo == 8 || eo == 1 || eo == 7 || eo == 2 || eo == 0 || eo == 48) ? eo : -1;
}

// Epilogue operands of one 16-pixel tile (addend, mask_y, mask_z), as loaded: the loads of ALL of a wave's tiles
// are issued before the first tile is processed (and, where registers allow, before the tile's MFMAs) -- issued
// tile by tile they cannot be hoisted over the previous tile's stores and every tile pays its own memory round
// trip (4 x 1.5 us in the block-end data gradient of a 256-pixel block).
template <int NTW>
struct EpiRaw {
    V16 ad[NTW], my[NTW], mz[NTW];   // bf16 wide path: NTW / 2 entries used; otherwise one per channel tile
};

template <typename T, int NTW, bool UNCOND = false, int EO = -1>
__device__ __forceinline__ void epilogue_fetch(const stl_conv& p, bool pok, size_t pix, int n0, int cbase, int g, EpiRaw<NTW>& e) {
    using O = EpiOps<EO>;
    if constexpr (sizeof(T) == 2 && NTW % 2 == 0) {
        // wide path: the lane's own 8-channel group per tile pair (same address as its store)
#pragma unroll
        for (int nj = 0; nj < NTW / 2; ++nj) {
            const int co = n0 + cbase + (2 * nj + (g & 1)) * 16 + 8 * (g >> 1);
            const size_t e8 = (pok && co < p.Co) ? pix + co : 0;  // invalid lanes read element 0; their values are masked later
            if constexpr (EO >= 0) {   // the operand set is known: exactly its loads
                if (O::mz(p)) e.mz[nj] = ldg16((const char*)p.mask_z + e8 * 2);
                if (O::ad(p)) e.ad[nj] = ldg16((const char*)p.addend + e8 * 2);
                if (O::my(p)) e.my[nj] = ldg16((const char*)p.mask_y + e8 * 2);
            } else if constexpr (UNCOND) {
                // straight-line: an absent operand reads the first bytes of the filter bank instead (always mapped, always
                // cached).  Branches around the loads make the wait-count insertion pessimistic (it drains these loads
                // before the next stage's loads are even issued).
                const char* bz = p.mask_z ? (const char*)p.mask_z + e8 * 2 : (const char*)p.w;
                const char* ba = p.addend ? (const char*)p.addend + e8 * 2 : (const char*)p.w;
                const char* by = p.mask_y ? (const char*)p.mask_y + e8 * 2 : (const char*)p.w;
                e.mz[nj] = ldg16(bz), e.ad[nj] = ldg16(ba), e.my[nj] = ldg16(by);
            } else {
                if (p.mask_z) e.mz[nj] = ldg16((const char*)p.mask_z + e8 * 2);
                if (p.addend) e.ad[nj] = ldg16((const char*)p.addend + e8 * 2);
                if (p.mask_y) e.my[nj] = ldg16((const char*)p.mask_y + e8 * 2);
            }
        }
    } else {
#pragma unroll
        for (int ni = 0; ni < NTW; ++ni) {
            const int co = n0 + cbase + ni * 16 + 4 * g;
            const size_t eo = (pok && co < p.Co) ? pix + co : 0;  // invalid lanes read element 0 and store nothing
            auto ld = [&](const void* base) __attribute__((always_inline)) {
                V16 v;
                if constexpr (sizeof(T) == 2) {
                    const uint2 u = *reinterpret_cast<const uint2*>((const char*)base + eo * 2);
                    v.w[0] = u.x, v.w[1] = u.y, v.w[2] = 0, v.w[3] = 0;
                } else {
                    v = ldg16((const char*)base + eo * 4);
                }
                return v;
            };
            if (O::mz(p)) e.mz[ni] = ld(p.mask_z);
            if (O::ad(p)) e.ad[ni] = ld(p.addend);
            if (O::my(p)) e.my[ni] = ld(p.mask_y);
        }
    }
}

// Fused epilogue of ONE 16-pixel tile of a wave: lane = pixel (lane & 15), channels 4g..4g+3 of each
// of the wave's NTW channel tiles (local channel base cbase).  +bias, +addend, ReLU mask of the
// producing BatchNorm (mask_y) with its yhat, ReLU, rounding to T, per-channel sums, stores.
//   pok: this lane's pixel exists; pix: its element offset (pixel * Co); n0: block's first channel.
//   s0/s1: running sums (out_stats: sum, sumsq; red: sum, sum*yhat) as packed pairs [NTW][2].
//   e: the tile's operands as fetched by epilogue_fetch.
// bf16 stores are widened with v_permlane16_swap: lanes g and g^1 exchange halves of two
// neighbouring channel tiles so that each lane stores 16 contiguous bytes.
// PLAIN: the launch has no bias / addend / mask operand (every forward convolution of the pose network): the operand
// code does not exist in that instantiation -- in particular no global load is issued in the epilogue, so no
// s_waitcnt vmcnt(0) stands between the accumulators and the stores (the counter is in order: waiting for a load
// issued HERE also waits for the next stage's staging loads, which were issued before it and are meant to stay in flight).
// TY: type of the FORWARD tensors among the operands (mask_y, mask_z); the addend and the output are T.
template <typename T, int NTW, int BCO, bool PLAIN = false, typename TY = T, int EO = -1>
__device__ __forceinline__ void epilogue_apply(const stl_conv& p, f32x4* acc, const float* cm, bool pok, size_t pix, int n0,
                                               int cbase, int g, f2v (*s0)[2], f2v (*s1)[2], const EpiRaw<NTW>& e) {
    using O = EpiOps<EO>;
    bool okv[NTW];
    size_t eov[NTW];
#pragma unroll
    for (int ni = 0; ni < NTW; ++ni) {
        const int co = n0 + cbase + ni * 16 + 4 * g;
        okv[ni] = pok && co < p.Co;
        eov[ni] = okv[ni] ? pix + co : 0;
    }
    f2v ad[NTW][2], my[NTW][2], mz[NTW][2];
    [[maybe_unused]] const float relu_thr = p.mask_bn.relu ? 0.f : -INFINITY;
    if constexpr (sizeof(T) == 2 && NTW % 2 == 0) {
#pragma unroll
        for (int nj = 0; nj < NTW / 2; ++nj) {
            if constexpr (!PLAIN) {
                if (O::mz(p)) unpack4p_pair<TY>(e.mz[nj], mz[2 * nj], mz[2 * nj + 1]);
                if (O::ad(p)) unpack4p_pair<T>(e.ad[nj], ad[2 * nj], ad[2 * nj + 1]);
                if (O::my(p)) unpack4p_pair<TY>(e.my[nj], my[2 * nj], my[2 * nj + 1]);
            }
        }
    } else {
#pragma unroll
        for (int ni = 0; ni < NTW; ++ni) {
            if constexpr (!PLAIN) {
                if (O::mz(p)) unpack4p<TY>(e.mz[ni], mz[ni][0], mz[ni][1]);
                if (O::ad(p)) unpack4p<T>(e.ad[ni], ad[ni][0], ad[ni][1]);
                if (O::my(p)) unpack4p<TY>(e.my[ni], my[ni][0], my[ni][1]);
            }
        }
    }
    uint32_t pk[NTW][2];   // bf16: the two packed dwords of this lane's 4 channels
    f2v fo[NTW][2];        // values as stored
#pragma unroll
    for (int ni = 0; ni < NTW; ++ni) {
        const int cl = cbase + ni * 16 + 4 * g;
        f2v f[2];
        f[0][0] = acc[ni][0], f[0][1] = acc[ni][1], f[1][0] = acc[ni][2], f[1][1] = acc[ni][3];
        if (!PLAIN && O::bias(p)) {
            const f2v* b2 = reinterpret_cast<const f2v*>(p.bias + (okv[ni] ? n0 + cl : 0));
            f[0] += b2[0], f[1] += b2[1];
        }
        if (!PLAIN && O::ad(p)) f[0] += ad[ni][0], f[1] += ad[ni][1];
        f2v yh[2] = {{0.f, 0.f}, {0.f, 0.f}};
        if (!PLAIN && O::my(p)) {
            const f2v* ma = reinterpret_cast<const f2v*>(cm + cl);
            const f2v* mb = reinterpret_cast<const f2v*>(cm + BCO + cl);
            const f2v* mm = reinterpret_cast<const f2v*>(cm + 2 * BCO + cl);
            const f2v* mr = reinterpret_cast<const f2v*>(cm + 3 * BCO + cl);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const f2v t = fma2(ma[h], my[ni][h], mb[h]);
                if constexpr (EO >= 0) {   // branch-free: the comparison's threshold is -inf when the BN has no ReLU
                    f[h][0] = t[0] > relu_thr ? f[h][0] : 0.f;
                    f[h][1] = t[1] > relu_thr ? f[h][1] : 0.f;
                } else if (p.mask_bn.relu) {
                    f[h][0] = t[0] > 0.f ? f[h][0] : 0.f;
                    f[h][1] = t[1] > 0.f ? f[h][1] : 0.f;
                }
                yh[h] = (my[ni][h] - mm[h]) * mr[h];
            }
        }
        if (!PLAIN && O::mz(p)) {  // gradient of z = ReLU(...): passes where z > 0
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                f[h][0] = mz[ni][h][0] > 0.f ? f[h][0] : 0.f;
                f[h][1] = mz[ni][h][1] > 0.f ? f[h][1] : 0.f;
            }
        }
        if (O::orelu(p)) {
#pragma unroll
            for (int h = 0; h < 2; ++h) f[h][0] = max_lo<T>(f[h][0], 0.f), f[h][1] = max_lo<T>(f[h][1], 0.f);
        }
        // round to the storage type once; statistics are those of the stored values
        if constexpr (sizeof(T) == 2) {
            const uint32_t keep = okv[ni] ? 0xFFFFFFFFu : 0u;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                pk[ni][h] = pack2<T>(f[h][0], f[h][1]) & keep;
                float lo_, hi_;
                unpack2<T>(pk[ni][h], lo_, hi_);
                fo[ni][h][0] = lo_, fo[ni][h][1] = hi_;
            }
        } else {
#pragma unroll
            for (int h = 0; h < 2; ++h) fo[ni][h][0] = okv[ni] ? f[h][0] : 0.f, fo[ni][h][1] = okv[ni] ? f[h][1] : 0.f;
        }
        if (O::ostats(p)) {
#pragma unroll
            for (int h = 0; h < 2; ++h) s0[ni][h] += fo[ni][h], s1[ni][h] += fo[ni][h] * fo[ni][h];
        } else if (!PLAIN && O::red(p)) {
#pragma unroll
            for (int h = 0; h < 2; ++h) s0[ni][h] += fo[ni][h], s1[ni][h] += fo[ni][h] * yh[h];
        }
        acc[ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if constexpr (sizeof(T) == 2) {
        if constexpr (NTW % 2 == 0) {
#pragma unroll
            for (int ni = 0; ni < NTW; ni += 2) {
                const auto sx = __builtin_amdgcn_permlane16_swap(pk[ni][0], pk[ni + 1][0], false, false);
                const auto sy = __builtin_amdgcn_permlane16_swap(pk[ni][1], pk[ni + 1][1], false, false);
                V16 v;
                v.w[0] = sx[0], v.w[1] = sy[0], v.w[2] = sx[1], v.w[3] = sy[1];
                const int co = n0 + cbase + (ni + (g & 1)) * 16 + 8 * (g >> 1);  // this lane's 8 channels
                if (pok && co < p.Co) stg16((char*)p.out + (pix + co) * 2, v);
            }
        } else {
#pragma unroll
            for (int ni = 0; ni < NTW; ++ni)
                if (okv[ni]) *reinterpret_cast<uint2*>((char*)p.out + eov[ni] * 2) = make_uint2(pk[ni][0], pk[ni][1]);
        }
    } else {
#pragma unroll
        for (int ni = 0; ni < NTW; ++ni) {
            if (okv[ni]) {
                V16 v;
                v.w[0] = __float_as_uint(fo[ni][0][0]), v.w[1] = __float_as_uint(fo[ni][0][1]);
                v.w[2] = __float_as_uint(fo[ni][1][0]), v.w[3] = __float_as_uint(fo[ni][1][1]);
                stg16((char*)p.out + eov[ni] * 4, v);
            }
        }
    }
}


// fetch + apply for one tile (callers that process a single tile at a time)
template <typename T, int NTW, int BCO, bool PLAIN = false, typename TY = T, int EO = -1>
__device__ __forceinline__ void epilogue_tile(const stl_conv& p, f32x4* acc, const float* cm, bool pok, size_t pix, int n0,
                                              int cbase, int g, f2v (*s0)[2], f2v (*s1)[2]) {
    EpiRaw<NTW> e;
    if constexpr (!PLAIN) epilogue_fetch<T, NTW, false, EO>(p, pok, pix, n0, cbase, g, e);
    epilogue_apply<T, NTW, BCO, PLAIN, TY, EO>(p, acc, cm, pok, pix, n0, cbase, g, s0, s1, e);
}

// Final reduction of the packed running sums: lanes of a 16-lane group hold the same channels.
template <int NTW>
__device__ __forceinline__ void xor_reduce_stats(f2v (*s0)[2], f2v (*s1)[2]) {
#pragma unroll
    for (int ni = 0; ni < NTW; ++ni)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                s0[ni][h][e] = row16_sum(s0[ni][h][e]), s1[ni][h][e] = row16_sum(s1[ni][h][e]);
            }
}
