// COCOeval.evaluateImg on gfx950, the part that does not depend on the pair metric: included by box_ap.hip (IoU, one workgroup per
// (image, category)) and keypoint_eval.hip (OKS, one workgroup per image) after common.cuh.  A kernel collects its rows, stages
// them, fills an fp64 tile [nd, ng] of its metric in LDS and ends in greedy_match; stl_box_ap_accumulate reads the slots of both.
//
// fp contract is off from here to the end of the including file, whether or not that file has said so already: every comparison
// below is with values computed exactly as written.
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;   // the match kernels and the NMS kernel (the sort strides by it); not box_ap_accumulate_kernel
static_assert(STL_BOX_AP_GT_MAX <= 128, "a chain keeps its matched flags in two 64-bit registers");

__host__ __device__ inline int pow2_at_least(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

// Ascending with the score in an unsigned integer of its width, -0 == +0, every NaN above +inf.
template <typename F>
__device__ __forceinline__ auto score_bits(F s) {
    using U = std::conditional_t<sizeof(F) == 4, uint32_t, uint64_t>;
    constexpr U top = (U)1 << (8 * sizeof(U) - 1), nan = sizeof(F) == 4 ? (U)0x7fc00000u : (U)0x7ff8000000000000ull;
    const U b = s == (F)0 ? (U)0 : (s != s ? nan : __builtin_bit_cast(U, s));
    return (U)((b & top) ? ~b : (b | top));
}

// Ascending bitonic sort of skey[0 .. m) padded to a power of two (padding sorts last); kPairs: of the pairs (skey, sidx).  Keys
// or pairs are unique, so this is a total order.  Every thread of the workgroup calls it.
template <bool kPairs>
__device__ __forceinline__ void bitonic_sort(uint64_t* skey, uint32_t* sidx, int m, int tid) {
    const int np = pow2_at_least(m);
    for (int p = m + tid; p < np; p += kThreads) {
        skey[p] = ~0ull;
        if constexpr (kPairs) sidx[p] = ~0u;
    }
    __syncthreads();
    for (int kk = 2; kk <= np; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < (np >> 1); i += kThreads) {
                const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo + j;
                const uint64_t x = skey[lo], y = skey[hi];
                bool gt = x > y;
                uint32_t xi = 0, yi = 0;
                if constexpr (kPairs) {
                    xi = sidx[lo], yi = sidx[hi];
                    gt = gt || (x == y && xi > yi);
                }
                if (gt == ((lo & kk) == 0)) {
                    skey[lo] = y, skey[hi] = x;
                    if constexpr (kPairs) sidx[lo] = yi, sidx[hi] = xi;
                }
            }
            __syncthreads();
        }
    }
}

// What a match kernel's arguments share; NT thresholds x NA area ranges are the chains, one lane each, bit t * NA + a of a slot.
template <int NT, int NA, typename Score>
struct MatchBase {
    static_assert(NT * NA <= 64, "one wave runs the chains and one 64-bit word per slot holds their bits");
    static constexpr int kThrs = NT, kAreas = NA;
    const int64_t* det_offsets;  // [I + 1]
    const int64_t* gt_offsets;   // [I + 1]
    int64_t N, G;
    int K, max_n, key_cap, max_g;
    double thr[NT], lo[NA], hi[NA];
    const Score* scores;         // [N]
    Score* slot_score;           // [N]
    int32_t* slot_cat;           // [N]
    int32_t* slot_rank;          // [N]
    uint64_t* slot_matched;      // [N]
    uint64_t* slot_ignored;      // [N]
    int32_t* npig;               // [I, K, NA]
};

// The offsets of an image the wrapper would have refused: the workgroup writes npig = -1 and leaves.
template <int NT, int NA, typename Score>
__device__ __forceinline__ bool offsets_refused(const MatchBase<NT, NA, Score>& a, int64_t o0, int64_t o1, int64_t g0, int64_t g1) {
    return o0 < 0 || o1 < o0 || o1 > a.N || o1 - o0 > a.max_n || g0 < 0 || g1 < g0 || g1 > a.G;
}

// Per area range (thread tid < NA): the ground truth with the non-ignored entries first, stable.  Ignored: the row's flag (a
// crowd, or whatever else the metric leaves out), or an area outside the range.
template <int NT, int NA, typename Score>
__device__ __forceinline__ void order_ground_truth(const MatchBase<NT, NA, Score>& a, const uint8_t* sgign, const double* sgarea, int ng,
                                                   uint8_t* sgord, int* s_npig, int32_t* npig_out, int tid) {
    if (tid >= NA) return;
    const double lo = a.lo[tid], hi = a.hi[tid];
    uint8_t* ord = sgord + tid * a.max_g;
    int c = 0;
    for (int g = 0; g < ng; ++g)
        if (!(sgign[g] || sgarea[g] < lo || sgarea[g] > hi)) ord[c++] = (uint8_t)g;
    s_npig[tid] = c;
    npig_out[tid] = c;
    for (int g = 0; g < ng; ++g)
        if (sgign[g] || sgarea[g] < lo || sgarea[g] > hi) ord[c++] = (uint8_t)g;
}

// The greedy match over the staged tile [nd, ng], by wave 0 after a barrier: lane c runs the chain of threshold c / NA and area
// range c % NA over the detections in score order; its matched flags (by position in that range's order) live in two registers.
// Detection d has the area det_area(d) and the image-local row det_row(d); its slot is base + d, in category k.
template <int NT, int NA, typename Score, typename Area, typename Row>
__device__ __forceinline__ void greedy_match(const MatchBase<NT, NA, Score>& a, const double* tile, const uint8_t* sgcrowd,
                                             const uint8_t* sgord, const int* s_npig, int nd, int ng, int64_t o0, int64_t base, int k,
                                             Area det_area, Row det_row, int lane) {
    const bool chain = lane < NT * NA;
    const int t = chain ? lane / NA : 0, ar = chain ? lane % NA : 0;
    const double thr0 = a.thr[t] < 1 - 1e-10 ? a.thr[t] : 1 - 1e-10;
    const double lo = a.lo[ar], hi = a.hi[ar];
    const uint8_t* ord = sgord + ar * a.max_g;
    const int nreg = s_npig[ar];          // positions >= nreg are the ignored ones
    const int walk = chain ? ng : 0;
    uint64_t gtm0 = 0, gtm1 = 0;
    for (int d = 0; d < nd; ++d) {
        double best = thr0;
        int mt = -1;
        for (int gi = 0; gi < walk; ++gi) {
            const int g = ord[gi];
            if ((((gi < 64 ? gtm0 : gtm1) >> (gi & 63)) & 1) && !sgcrowd[g]) continue;   // already matched, and not a crowd
            if (mt > -1 && mt < nreg && gi >= nreg) break;                                  // matched a regular one: stop at the ignored
            const double v = tile[d * ng + g];
            if (v < best) continue;
            best = v, mt = gi;                                                              // a tie moves to the later ground truth
        }
        bool ign;
        if (mt > -1) {
            ign = mt >= nreg;
            if (mt < 64) gtm0 |= 1ull << mt;
            else gtm1 |= 1ull << (mt - 64);
        } else {
            const double da = det_area(d);
            ign = da < lo || da > hi;
        }
        const uint64_t mb = __ballot(chain && mt > -1), ib = __ballot(chain && ign);
        if (lane == 0) {
            a.slot_score[base + d] = a.scores[o0 + det_row(d)];
            a.slot_cat[base + d] = k;
            a.slot_rank[base + d] = d;
            a.slot_matched[base + d] = mb;
            a.slot_ignored[base + d] = ib;
        }
    }
}

}  // namespace

// What both match entry points do once their arguments are checked: thresholds and area ranges into the kernel's arguments, the
// key capacity, the kernel's dynamic-LDS limit (lds_of(a) bytes) and one launch per 2^20 images (grid.x is the image: any number of
// them; grid.y the K categories).
template <typename Args, typename Lds>
static inline int launch_match(const char* name, void (*kernel)(Args), Args& a, const double* thrs, const double* area_ranges, int max_n,
                               int max_g, int num_images, int K, Lds lds_of, hipStream_t st) {
    constexpr int NT = Args::kThrs, NA = Args::kAreas;
    a.K = K, a.max_n = max_n, a.max_g = max_g > 0 ? max_g : 1, a.key_cap = pow2_at_least(max_n > 0 ? max_n : 1);
    for (int t = 0; t < NT; ++t) a.thr[t] = thrs[t];
    for (int r = 0; r < NA; ++r) a.lo[r] = area_ranges[2 * r], a.hi[r] = area_ranges[2 * r + 1];
    const size_t lds = lds_of(a);
    const hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    STL_CHECK(ea == hipSuccess, "%s: %zu bytes of dynamic LDS refused (max_n = %d, max_g = %d): %s", name, lds, max_n, max_g,
              hipGetErrorString(ea));
    for (int i0 = 0; i0 < num_images; i0 += 1 << 20) {
        Args b = a;
        const int ni = num_images - i0 < (1 << 20) ? num_images - i0 : (1 << 20);
        b.det_offsets += i0, b.gt_offsets += i0, b.npig += (size_t)i0 * K * NA;
        STL_LAUNCH(kernel, dim3(ni, K), dim3(kThreads), lds, st, b);
        STL_LAUNCH_CHECK(name);
    }
    return 0;
}
