// les_hip_march_tables.inc -- part of the single translation unit les_hip.hip: the kernel instantiations compiled into this build
// ---- kernel configurations compiled into this build: guided-filter radius -> strip geometry
typedef void (*StripKernel)(les::Geom, les::View, const les::Job*, const float4*, float*, int, int);
struct StripEntry { int R; int variant; int TW; int NT; StripKernel fn; };

// (radius, stage-1 columns WA, rows per block BY, H-phase segments SEG, min waves/SIMD MW); variant 0 is
// the default of a radius, the others are selectable with LES_HIP_VARIANT for A/B measurements.
#define LES_STRIP_ENTRY(R_, V_, WA_, BY_, SEG_, MW_) \
    { R_, V_, les::StripCfg<R_, WA_, BY_, SEG_>::TW, les::StripCfg<R_, WA_, BY_, SEG_>::NT, les::les_strip_kernel<R_, WA_, BY_, SEG_, MW_> }
const StripEntry kStrips[] = {
    // Defaults per radius.  Measured on MI355X (R = 10, 1500x1000x256): occupancy without register spills wins --
    // (WA 64, BY 21 = ring length, SEG 3, 3 waves/SIMD, 0 B scratch) 7.0 ms vs 9.2 ms for (128,16,8,2 waves) and
    // 12+ ms for anything that spills.
    LES_STRIP_ENTRY(1, 0, 64, 16, 4, 2), LES_STRIP_ENTRY(2, 0, 64, 16, 4, 2), LES_STRIP_ENTRY(3, 0, 64, 16, 4, 2),
    LES_STRIP_ENTRY(4, 0, 64, 16, 4, 2), LES_STRIP_ENTRY(5, 0, 64, 16, 4, 2), LES_STRIP_ENTRY(6, 0, 64, 16, 4, 2),
    LES_STRIP_ENTRY(7, 0, 64, 16, 4, 2), LES_STRIP_ENTRY(8, 0, 64, 16, 4, 2), LES_STRIP_ENTRY(9, 0, 64, 16, 4, 2),
    LES_STRIP_ENTRY(10, 0, 64, 21, 3, 3), LES_STRIP_ENTRY(12, 0, 64, 16, 4, 2), LES_STRIP_ENTRY(15, 0, 96, 16, 6, 2),
    // A/B variants for radius 10 (LES_HIP_VARIANT=n)
    // Kept: the wide strip and the default geometry at 2 waves/SIMD.  Measured earlier in the round (ms per 1500x1000x256 pass,
    // default then 7.14): (64,21,3) at 2 waves/SIMD 9.57 | (128,21,SEG 3/4/6) at 2 waves 10.2 / 11.2 / 8.8 | (128,16,8) 9.6 |
    // (96,21,SEG 3/4) at 2 waves (6-wave workgroups) 15.1 / 12.4 | (80,21,3) 14.4 | anything that spills 11-15:
    // occupancy beats the lower instruction count of wide strips
    LES_STRIP_ENTRY(10, 8, 128, 21, 6, 2), LES_STRIP_ENTRY(10, 11, 64, 21, 3, 2),
};
// image-based matching cost (les_hip_create_naive): one conservative configuration per radius
#define LES_NAIVE_ENTRY(R_, WA_, BY_, SEG_, MW_) \
    { R_, 0, les::StripCfg<R_, WA_, BY_, SEG_>::TW, les::StripCfg<R_, WA_, BY_, SEG_>::NT, les::les_strip_kernel<R_, WA_, BY_, SEG_, MW_, 1> }
const StripEntry kNaiveStrips[] = {
    LES_NAIVE_ENTRY(1, 64, 16, 4, 2), LES_NAIVE_ENTRY(2, 64, 16, 4, 2), LES_NAIVE_ENTRY(3, 64, 16, 4, 2), LES_NAIVE_ENTRY(4, 64, 16, 4, 2),
    LES_NAIVE_ENTRY(5, 64, 16, 4, 2), LES_NAIVE_ENTRY(6, 64, 16, 4, 2), LES_NAIVE_ENTRY(7, 64, 16, 4, 2), LES_NAIVE_ENTRY(8, 64, 16, 4, 2),
    LES_NAIVE_ENTRY(9, 64, 16, 4, 2), LES_NAIVE_ENTRY(10, 64, 16, 4, 2), LES_NAIVE_ENTRY(12, 64, 16, 4, 2), LES_NAIVE_ENTRY(15, 96, 16, 6, 2),
};
// cost volume at interpolation 0 / 2 (setInterpolationMethod, les_hip_set_interpolation): the exact per-pixel gathers, the same
// conservative configuration per radius.  They serve every fall-back of those modes and recompute the flagged calls of a march launch.
#define LES_INTERP_ENTRY(R_, WA_, BY_, SEG_, MW_, SRC_) \
    { R_, 0, les::StripCfg<R_, WA_, BY_, SEG_>::TW, les::StripCfg<R_, WA_, BY_, SEG_>::NT, les::les_strip_kernel<R_, WA_, BY_, SEG_, MW_, SRC_> }
#define LES_INTERP_ENTRIES(SRC_) \
    LES_INTERP_ENTRY(1, 64, 16, 4, 2, SRC_), LES_INTERP_ENTRY(2, 64, 16, 4, 2, SRC_), LES_INTERP_ENTRY(3, 64, 16, 4, 2, SRC_), \
    LES_INTERP_ENTRY(4, 64, 16, 4, 2, SRC_), LES_INTERP_ENTRY(5, 64, 16, 4, 2, SRC_), LES_INTERP_ENTRY(6, 64, 16, 4, 2, SRC_), \
    LES_INTERP_ENTRY(7, 64, 16, 4, 2, SRC_), LES_INTERP_ENTRY(8, 64, 16, 4, 2, SRC_), LES_INTERP_ENTRY(9, 64, 16, 4, 2, SRC_), \
    LES_INTERP_ENTRY(10, 64, 16, 4, 2, SRC_), LES_INTERP_ENTRY(12, 64, 16, 4, 2, SRC_), LES_INTERP_ENTRY(15, 96, 16, 6, 2, SRC_)
const StripEntry kNearestStrips[] = { LES_INTERP_ENTRIES(2) };
const StripEntry kQuadraticStrips[] = { LES_INTERP_ENTRIES(3) };
// interp 0: nearest, 2: quadratic
const StripEntry* find_interp_strip(int R, int interp)
{
    for (const auto& e : (interp == 0 ? kNearestStrips : kQuadraticStrips))
        if (e.R == R) return &e;
    return nullptr;
}
const StripEntry* find_naive_strip(int R)
{
    for (const auto& e : kNaiveStrips)
        if (e.R == R) return &e;
    return nullptr;
}
const StripEntry* find_strip(int R)
{
    int variant = 0;
    if (const char* v = getenv("LES_HIP_VARIANT")) variant = atoi(v);
    const StripEntry* def = nullptr;
    for (const auto& e : kStrips) {
        if (e.R != R) continue;
        if (e.variant == variant) return &e;
        if (e.variant == 0) def = &e;
    }
    return def;
}

// ---- the fixed-point march kernel (les_march.h): (radius, columns per job slot, job slots per workgroup, rows per block)
typedef void (*MarchKernel)(les::Geom, les::MarchView, const les::Job*, const float4*, float*, int, int);
struct MarchEntry { int R; int TW; int NJ; int NT; int BY; MarchKernel fn; };
#define LES_MARCH_ENTRY(R_, WGC_, NJ_, BY_) \
    { R_, les::MarchCfg<R_, WGC_, NJ_, BY_>::TW, NJ_, les::MarchCfg<R_, WGC_, NJ_, BY_>::NT, BY_, les::les_march_kernel<R_, WGC_, NJ_, BY_> }
// two geometries per radius: wide jobs (WGC - 4R output columns: whole-image hypothesis slabs, layer-1/2 cells) and two narrow jobs
// per workgroup (128 - 4R output columns each: layer-0 cells); both run 12 waves per workgroup.
// Radii 2 .. 10 (windR 4 .. 21; the reference's option -filterRadious, LES/main.cpp:48,285,349; its default 20 -> radius 10).  Radii 2 and 3 since round 6
// (64 planes of 1500 x 1000: 1.11 / 0.85 ms against 1.23 / 1.25 ms on the strip kernel); radius 1 -- a ring of three rows, one row per tick -- was measured
// slower than the strip kernel (1.88 against 1.80 ms, tools/lab/radius_time.py) and stays there.  The rings
// hold RS = 3 x BY >= 2R + 1 rows (three ticks per unrolled loop iteration, three stage-2 buffers; the row that leaves a window is read
// from slot (s + RS - (2R + 1)) mod RS), with BY <= 8 rows per prefix pass: the smallest such block height per radius.  Radius 11 would
// need BY = 8 and 176 KB of LDS, radius 12 and beyond more than 24 ring rows: they stay on the strip kernel.
const MarchEntry kMarch[] = {
    LES_MARCH_ENTRY(10, 256, 1, 7),
#if defined(LES_MARCH_LAB) && defined(LES_MARCH_NARROW_NJ1)
    LES_MARCH_ENTRY(10, 128, 1, 7),          // experiment: one narrow job per workgroup, two workgroups per CU (independent tick barriers)
#else
    LES_MARCH_ENTRY(10, 128, 2, 7),
#endif
    LES_MARCH_ENTRY(7, 256, 1, 5),
    LES_MARCH_ENTRY(7, 128, 2, 5),
#if !defined(LES_MARCH_FEW_RADII)
    LES_MARCH_ENTRY(2, 256, 1, 2),  LES_MARCH_ENTRY(2, 128, 2, 2),
    LES_MARCH_ENTRY(3, 256, 1, 3),  LES_MARCH_ENTRY(3, 128, 2, 3),
    LES_MARCH_ENTRY(4, 256, 1, 3),  LES_MARCH_ENTRY(4, 128, 2, 3),
    LES_MARCH_ENTRY(5, 256, 1, 4),  LES_MARCH_ENTRY(5, 128, 2, 4),
    LES_MARCH_ENTRY(6, 256, 1, 5),  LES_MARCH_ENTRY(6, 128, 2, 5),
    LES_MARCH_ENTRY(8, 256, 1, 6),  LES_MARCH_ENTRY(8, 128, 2, 6),
    LES_MARCH_ENTRY(9, 256, 1, 7),  LES_MARCH_ENTRY(9, 128, 2, 7),
#endif
};
// wide != 0: the entry with the widest jobs, else the one with the narrowest
const MarchEntry* find_march(int R, int wide = 1)
{
    if (const char* k = getenv("LES_HIP_KERNEL")) if (!strcmp(k, "strip")) return nullptr;     // A/B measurements: force the fp64 strip kernel
    const MarchEntry* best = nullptr;
    for (const auto& e : kMarch)
        if (e.R == R && (!best || (wide ? e.TW > best->TW : e.TW < best->TW))) best = &e;
    return best;
}

constexpr long long kRawPatchCapFloats = 1ll << 30;   // 4 GB of raw-cost patches per batch and view (image-based energy on the march kernel)
constexpr int kRansacMaxSam = 500;   // RansacProposer default MAX_SAM, LES/Proposer.h:265
constexpr int kRansacChunks = 5;
constexpr int kRansacChunkEnds[kRansacChunks] = {16, 64, 128, 256, kRansacMaxSam};   // the candidates are evaluated in chunks that end here (les_propose.h)

