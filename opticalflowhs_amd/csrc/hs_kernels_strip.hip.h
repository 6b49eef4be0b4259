// hs_kernels_strip.hip.h -- the register-resident multi-sweep Jacobi kernels (k_jacobi_strip, the default, and
// its folded form k_jacobi_fold).  Included by hs_kernels.hip.h, which holds the shared arithmetic.
#pragma once
#include <type_traits>

// Last sweep of a launch as a second copy of the sweep code after the loop (the loop then publishes and
// meets the barrier unconditionally), in both kernels (run_sweeps).  Folded kernel: far fewer spills (R = 4: 33 -> 7,
// R = 5: 33 -> 1) and 15 VGPRs less at R = 3, and with two sweeps per loop trip the register copies at the loop's back
// edge halve (profiles/r01_fold_peel_ab.txt, r01_fold_unroll2_ab.txt); strip kernel: the compiler ended every loop trip
// with 44 - 64 register copies until the last sweep was peeled out of the loop, after which 4 remain.
// Scaled state: inside a launch the flow is carried as 4^k * u after k sweeps, so that the neighbour SUM is
// the average at the next scale and the multiplication by 0.25 disappears (the constant term ga is rescaled
// instead: one packed multiply per pair of pixels where there were two).  Powers of 4 commute with every
// rounding, so the result is bit-identical to the canonical arithmetic of update_cv<> -- except for values that
// would be denormal there (below 1.2e-38), which keep their bits here.  A launch has up to kMaxFuse = 32 sweeps, so the
// state reaches 4^33 = 7.4e19 times the flow: no overflow for the flow the solver itself makes from zero while
// lambda <= 1e20 (beyond that the host keeps launches to 8 sweeps), but the kernels do NOT bound the flow they are
// handed.  For planes a caller wrote, or that a solve with a larger lambda left, the host measures the largest |value|
// and caps the launch length (flow_launch_cap, hs_solve.hip.h); values from about 5e36 go to the one-sweep kernel.
// NaN and Inf need no care: they spread through the scaled state exactly as through the canonical one.
#ifndef HS_SWEEP_STAMPS
#define HS_SWEEP_STAMPS 0
#endif
#ifndef HS_DIAG /* bit mask of diagnostic knobs in the strip sweep (timing experiments only, results are wrong): 1 no LDS
                   exchange, 2 no barrier, 4 no trapezoid gating, 8 no arithmetic */
#define HS_DIAG 0
#endif


namespace hsk {

// ------------------------------------------------------------------------------------------
// a2, form 3: T Jacobi sweeps per launch on register-resident strips ("strip").
//
// A workgroup of NW wavefronts owns a region of 256 columns x (NW*R) rows.  Wavefront w holds rows
// [w*R, (w+1)*R) entirely in VGPRs: lane l owns the 4 pixels of columns 4l..4l+3 in each of its R
// rows (u, v and the four coefficients).  Per sweep:
//   * left/right neighbours come from lanes l-1 / l+1 by DPP wave shifts (the wavefront spans the
//     whole region width, so there is no seam: lanes 0 and 63 sit on the region edge);
//   * up/down neighbours inside the strip are the lane's own registers;
//   * only the strip's first and last row go through LDS (double-buffered, ONE barrier per sweep)
//     to reach the wavefronts above and below.
// LDS traffic per sweep is 2 of R rows instead of all of them and nothing is re-read, so the sweep
// is bound by VALU issue (~13 flops per pixel) rather than by LDS or barriers.
//
// Image borders cost nothing inside the sweep loop: Jacobi with a replicate border is exactly
// Jacobi on the EVEN REFLECTION of the image (u(-1-k) = u(k), same for the coefficients): the
// mirrored pixel sees the mirrored neighbour set, so the extension stays a reflection sweep after
// sweep, bit for bit, and pixel 0's left neighbour u(-1) equals u(0) -- the replicate rule.  So the
// halo outside the image is simply LOADED from mirrored coordinates and then swept like any other
// pixel; no select, no ghost copy.
// ------------------------------------------------------------------------------------------
struct StripGeom {
    int W, H, P;
    long long plane;
    int T, HX;          // sweeps per launch; horizontal halo (multiple of 4, >= T)
    int CW, CH;         // core = (256 - 2*HX) x (NW*R - 2*T)
    int NW;             // wavefronts per workgroup
    int tiles_x, tiles_y;
    int zero_in;        // incoming flow is identically zero: u_in = v_in = ONE row of zeros (at least P floats), read with pitch 0
    int org;            // frame row of this context's row 0, modulo 2 (row slabs; checkerboard phase of update_cv)
    int ey0, ey1;       // rows [ey0, ey1) of the context whose changes count for Eps and the witness (hsflow_set_eps_rows: a row slab's
                        // owned rows -- its halo rows repeat a neighbour's, stale towards the slab's edge); the strip kernel only
    const int *pair_list; // NULL: workgroups [k * tiles_x * tiles_y, ...) work on pair k.  Else a device array of pair indices: they work
                        // on pair pair_list[k] (the per-pair stop's launches over the pairs that are still running).  Read once per
                        // workgroup, ahead of the load phase (a scalar load; only the pair's plane offset lives on)
};

// index of the even reflection: ..., 1, 0 | 0, 1, ..., n-1 | n-1, n-2, ...
__device__ __forceinline__ int mirror_index(int i, int n)
{
    if (i < 0) i = -1 - i;            // one bounce covers every image at least as large as the halo
    if (i >= n) i = 2 * n - 1 - i;
    if ((unsigned)i >= (unsigned)n) { // tiny image: general even-periodic extension
        const int p = 2 * n;
        int m = i % p;
        if (m < 0) m += p;
        i = m < n ? m : p - 1 - m;
    }
    return i;
}

typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------
// The persistent form of the strip kernel (k_jacobi_strip_persist): ONE launch for a whole solve.  Every workgroup
// keeps its region's coefficients and flow in registers across PHASES of T sweeps; between two phases it publishes its
// core tile (write-through stores), raises its tile's phase counter, waits for the counters of its 8 neighbours and
// reloads only the halo pixels of its region -- no kernel boundary, no second read of the coefficients, no second
// v_rsq per pixel.  Replaces the host loop of HSOpticalFlowOpenCL.cpp:748-752 at the level of one kernel.
// Hand-off protocol (MI355X_MICROARCH.md, inter-workgroup visibility, first row of the table): every byte handed over
// is stored with `sc1` (write-through) and loaded with `sc1` (L1 bypass); every storing wave drains its stores
// (s_waitcnt vmcnt(0)), the workgroup meets at a barrier, ONE lane then stores the counter `sc1`; the consumer polls
// with `sc1` loads from one wave and the other waves load after a workgroup barrier that wave joins.
// All workgroups must be resident at once (the host checks occupancy x CUs >= grid); every wait is bounded in time:
// a workgroup that gives up writes the error word and an abort word the others watch, and returns.
// ------------------------------------------------------------------------------------------
struct PersistArgs {
    unsigned *flags;        // [tiles] phases published by each tile, counted up across solves; [tiles] = abort word
    unsigned *err;          // error word in page-locked host memory: 1 = a wait timed out (results invalid)
    float *ub[2], *vb[2];   // phase p publishes into buffer p & 1; the last phase's buffer is the solve's output
    int n_phase, T_last;    // phases of the solve; sweeps of the last one (all others run g.T)
    unsigned wait_ticks;    // a wait gives up after this many 100 MHz ticks
};

// The hand-off's 16-byte accesses as raw buffer instructions with the sc1 bit (aux 16: write-through store, L1-bypassing
// load): the address is a scalar row offset + a per-lane byte offset, so no 64-bit vector arithmetic, and -- unlike
// inline assembly -- the compiler keeps track of the loads in flight.  One descriptor per plane (no bounds: the
// offsets are those of the ordinary loads and stores).
typedef unsigned u4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t plane_rsrc(float *p)
{
    return __builtin_amdgcn_make_buffer_rsrc((void *)p, 0, 0xFFFFFFFFu, 0x00020000);
}
__device__ __forceinline__ void store_f4_sc1(__amdgpu_buffer_rsrc_t rs, unsigned row_bytes, unsigned lane_bytes, f4 v)
{
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4v, v), rs, (int)lane_bytes, (int)row_bytes, 16);
}
__device__ __forceinline__ f4 load_f4_sc1(__amdgpu_buffer_rsrc_t rs, unsigned row_bytes, unsigned lane_bytes)
{
    return __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)lane_bytes, (int)row_bytes, 16));
}
__device__ __forceinline__ unsigned load_u32_sc1(const unsigned *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The lane number from the hardware, at the point of use (two instructions): a register holding it across the sweep loop
// is one the R = 5 kernels do not have (the mask goes through an empty asm so that the optimiser cannot hoist the pair).
__device__ __forceinline__ int hs_lane_now()
{
    unsigned m = ~0u;
    asm volatile("" : "+s"(m));
    return (int)__builtin_amdgcn_mbcnt_hi(m, __builtin_amdgcn_mbcnt_lo(m, 0u));
}

__device__ __forceinline__ f2 f2_fma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f2 f2_swap(f2 a) { return __builtin_shufflevector(a, a, 1, 0); }
// old - new of a sweep, in the NEW value's scale (scaled state: the old one is a factor 4 behind)
__device__ __forceinline__ f2 sweep_diff(f2 o, f2 n) { return f2_fma(o, f2{4.0f, 4.0f}, -n); }
__device__ __forceinline__ float sweep_diff(float o, float n) { return fmaf(4.0f, o, -n); }

// One row of one lane: pixels (p0,p3) = P and (p1,p2) = Q as two register pairs (p0 is an even image column: the
// region starts at a multiple of 4), so that all arithmetic is packed (2 pixels per v_pk_add/mul/fma_f32; cross_rows).
struct RowCoef { f2 alP, alQ, beP, beQ, gaP, gaQ; };

// The canonical 4-neighbour sum (update_cv, hs_kernels.hip.h) adds two diagonal pairs chosen by the pixel's
// checkerboard parity.  Every such pair straddles one row boundary and belongs to two pixels, so it is formed ONCE:
//   cross sum of the boundary between rows r and r+1, at pixel i of row r:
//       s_r[i] = x[r+1][i] + x[r][i+1]   (pixel (r,i) even)        s_r[i] = x[r+1][i] + x[r][i-1]   (odd)
//   neighbour sum of pixel (r,i):  s_r[i] + s_(r-1)[i-1]  (even)   s_r[i] + s_(r-1)[i+1]  (odd)
// A lane's four pixels p0..p3 of a row live in the two register pairs P = (p0, p3) and Q = (p1, p2).  With E = parity
// of pixel p0 of the upper row: for E = 0 every pixel's partner lies in the lane's OTHER pair (two plain packed adds);
// for E = 1 the inner pixels p1, p2 are each other's partners (one packed add with swapped halves) and the outer ones
// reach into the adjacent lanes (two DPP adds); the neighbour sum is the other way round.  Rows alternate, so a row
// costs 3 packed + 2 DPP adds per plane and no unpacked one (pairing (p0, p1), (p2, p3): 2 packed + 2 DPP + 2 plain;
// the straightforward sum: 4 + 2 + 2).
struct Cross { f2 uP, uQ, vP, vQ; };

// a + swap(b) in one packed add (written out: left to the compiler, the swap of a row that has just come from LDS is
// done with two moves first)
__device__ __forceinline__ f2 pk_add_swapped(f2 a, f2 b)
{
    f2 r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// s of the boundary below row `c` (whose side neighbours it uses; `d` is the row underneath), E = parity of c's p0
template <int E>
__device__ __forceinline__ void cross_rows(Cross &s, const f2 cuP, const f2 cuQ, const f2 cvP, const f2 cvQ,
                                           const f2 duP, const f2 duQ, const f2 dvP, const f2 dvQ)
{
    if (E == 0) { // p0 + c1, p3 + c2 | p1 + c0, p2 + c3
        s.uP = duP + cuQ; s.uQ = duQ + cuP;
        s.vP = dvP + cvQ; s.vQ = dvQ + cvP;
    } else {      // p1 + c2, p2 + c1 | p0 + previous lane's c3, p3 + next lane's c0
        s.uQ = pk_add_swapped(duQ, cuQ);
        s.uP.x = duP.x + wave_from_prev_lane(cuP.y); s.uP.y = duP.y + wave_from_next_lane(cuP.x);
        s.vQ = pk_add_swapped(dvQ, cvQ);
        s.vP.x = dvP.x + wave_from_prev_lane(cvP.y); s.vP.y = dvP.y + wave_from_next_lane(cvP.x);
    }
}

// One row: neighbour sums from the cross sums below (sc) and above (sp) it, then the update in place.
// E = parity of the row's p0.  Scaled state: the sums ARE the averages at the next scale (file header).
template <int E>
__device__ __forceinline__ void strip_row_update(f2 &uP, f2 &uQ, f2 &vP, f2 &vQ, const Cross &sc, const Cross &sp, RowCoef &c)
{
    f2 ubP, ubQ, vbP, vbQ; // 4^(k+1) * average
    if (E == 0) {
        ubQ = pk_add_swapped(sc.uQ, sp.uQ);
        ubP.x = sc.uP.x + wave_from_prev_lane(sp.uP.y); ubP.y = sc.uP.y + wave_from_next_lane(sp.uP.x);
        vbQ = pk_add_swapped(sc.vQ, sp.vQ);
        vbP.x = sc.vP.x + wave_from_prev_lane(sp.vP.y); vbP.y = sc.vP.y + wave_from_next_lane(sp.vP.x);
    } else {
        ubP = sc.uP + sp.uQ; ubQ = sc.uQ + sp.uP;
        vbP = sc.vP + sp.vQ; vbQ = sc.vQ + sp.vP;
    }
    const f2 qP = f2_fma(c.alP, ubP, f2_fma(c.beP, vbP, c.gaP));
    const f2 qQ = f2_fma(c.alQ, ubQ, f2_fma(c.beQ, vbQ, c.gaQ));
    uP = f2_fma(-c.alP, qP, ubP);
    vP = f2_fma(-c.beP, qP, vbP);
    uQ = f2_fma(-c.alQ, qQ, ubQ);
    vQ = f2_fma(-c.beQ, qQ, vbQ);
    c.gaP *= 4.0f; // the constant term at the next sweep's scale
    c.gaQ *= 4.0f;
}

// The packed derivative words of a lane's R rows straight from the two frames (DERIV launches: the first
// launch of a solve then needs no separate derivative pass).  Same arithmetic as k_deriv_cv, on the EVEN
// REFLECTION of frame A -- which is the replicate border at the image edge (A(-1) = A(0)) and, further out,
// yields the derivative of the mirrored pixel with the sign of the component across the mirror flipped; the
// flip is undone here because the halo wants the mirrored pixel's coefficients unchanged.  The column
// neighbours x0-1 and x0+4 come from the adjacent lanes (the region is contiguous in the reflected image);
// lanes 0 and 63 have none, so the region's outermost columns get a wrong Ix -- they are invalid after the
// first sweep anyway (HX >= T >= 1).  Host-side condition (strip_deriv_fusable): the image is at least as
// large as the region, so that one bounce suffices.
// Register row r of the lane is image row y0 + dir * r (dir = -1: the folded kernel's lower half, whose
// registers run bottom-up).
// FrameSrc (the strip kernel's launches): the frames may lie in the CALLER's planes, with row pitches of their own; the
// lanes named by `keep` (bit r: register row r is a core row of a core lane) then store the frame words of their rows
// into the context's planes as soon as they have arrived -- the first launch of a stream submission replaces the frame
// copy (hsflow_solve_async_frames_device).
struct FrameSrc {
    int PA, PB;             // row pitches of fA / fB in bytes (the context's own planes: g.P)
    uint8_t *keepA, *keepB; // the context's frame planes when fA / fB are the caller's, else NULL: nothing is stored
};

template <int R, bool EXT = false>
__device__ __forceinline__ void strip_derive(const uint8_t *__restrict__ fA, const uint8_t *__restrict__ fB,
                                             const StripGeom &g, long long base, int x0, int y0, int dir, bool xin,
                                             uint4 (&lc)[R], const FrameSrc fs = FrameSrc{0, 0, nullptr, nullptr},
                                             const unsigned keep = 0)
{
    const int PA = EXT ? fs.PA : g.P, PB = EXT ? fs.PB : g.P;
    // How this lane reads its four columns of a frame row: 0 an aligned word (group inside the image), 1 an
    // aligned word read backwards (group wholly mirrored: left of the image, or right of it when W % 4 == 0),
    // 2 four reflected bytes (W % 4 != 0: the group that straddles column W-1 and those right of it).
    // (column_rule, below, states the same rule for the flow and coefficient loads: mode 1 is its rev, mode 2 its slow.
    // Whether strip_derive compiles the same with it has not been tried; the rule stays written out here.)
    const int mode = xin ? 0 : ((x0 < 0 || (g.W & 3) == 0) ? 1 : 2);
    int xg = x0, xb[4] = {0, 0, 0, 0};
    unsigned flipx = 0; // pixels of the group that are mirrored columns: their Ix changes sign
    if (mode == 1) {
        xg = x0 < 0 ? -x0 - 4 : 2 * g.W - x0 - 4;
        if (xg < 0 || xg + 4 > g.W) xg = 0; // excluded by the host; keeps the load inside the row regardless
        flipx = 0xFu;
    } else if (mode == 2) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            xb[k] = mirror_index(x0 + k, g.W);
            if (x0 + k >= g.W) flipx |= 1u << k;
        }
    }
    // All word loads first, branch-free (mode 2 lanes read a harmless aligned word), so that they overlap;
    // then ONE wave-uniform branch in which the mode 2 lanes -- if the wavefront has any -- fetch their bytes.
    uint32_t wa[R + 2], wbv[R];
#pragma unroll
    for (int j = 0; j < R + 2; j++)
        wa[j] = *(const uint32_t *)(fA + base + (long long)mirror_index(y0 + dir * (j - 1), g.H) * PA + (mode == 2 ? 0 : xg));
#pragma unroll
    for (int r = 0; r < R; r++)
        wbv[r] = *(const uint32_t *)(fB + base + (long long)mirror_index(y0 + dir * r, g.H) * PB + (mode == 2 ? 0 : xg));
    if (mode == 1) {
#pragma unroll
        for (int j = 0; j < R + 2; j++) wa[j] = __builtin_bswap32(wa[j]);
#pragma unroll
        for (int r = 0; r < R; r++) wbv[r] = __builtin_bswap32(wbv[r]);
    }
    if (__builtin_amdgcn_ballot_w64(mode == 2) != 0) {
        if (mode == 2) {
            auto bytes = [&](const uint8_t *row) -> uint32_t {
                return (uint32_t)row[xb[0]] | ((uint32_t)row[xb[1]] << 8) | ((uint32_t)row[xb[2]] << 16) | ((uint32_t)row[xb[3]] << 24);
            };
#pragma unroll
            for (int j = 0; j < R + 2; j++) wa[j] = bytes(fA + base + (long long)mirror_index(y0 + dir * (j - 1), g.H) * PA);
#pragma unroll
            for (int r = 0; r < R; r++) wbv[r] = bytes(fB + base + (long long)mirror_index(y0 + dir * r, g.H) * PB);
        }
    }
    if constexpr (EXT) {
        // The frames are the caller's: the core lanes leave the context's own copy behind (the cores tile the image, and no
        // workgroup of this launch reads those planes; mirrored groups are never core lanes).  A group that straddles
        // column W-1 stores reflected bytes into the row's padding, which nothing reads.
        if (fs.keepA != nullptr) { // launch-uniform
#pragma unroll
            for (int r = 0; r < R; r++) {
                if ((keep >> r) & 1u) {
                    const long long o = base + (long long)(y0 + dir * r) * g.P + x0;
                    *(uint32_t *)(fs.keepA + o) = wa[r + 1];
                    *(uint32_t *)(fs.keepB + o) = wbv[r];
                }
            }
        }
    }
    int a[R + 2][6]; // columns x0-1 .. x0+4 of the reflected rows y0 - dir, y0, ..., y0 + dir * R
#pragma unroll
    for (int j = 0; j < R + 2; j++) {
        const uint32_t wd = wa[j];
        a[j][0] = (int)((uint32_t)__builtin_amdgcn_update_dpp(0, (int)wd, 0x138, 0xF, 0xF, true) >> 24);
        a[j][5] = (int)((uint32_t)__builtin_amdgcn_update_dpp(0, (int)wd, 0x130, 0xF, 0xF, true) & 0xFFu);
#pragma unroll
        for (int k = 0; k < 4; k++) a[j][k + 1] = (int)((wd >> (8 * k)) & 0xFFu);
    }
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int y = y0 + dir * r;
        const uint32_t wb = wbv[r];
        const bool yflip = (y < 0 || y >= g.H) != (dir < 0); // a[r + 2] is the row BELOW only when dir > 0
        uint32_t o[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            int ix8 = (a[r][k + 2] + 2 * a[r + 1][k + 2] + a[r + 2][k + 2]) - (a[r][k] + 2 * a[r + 1][k] + a[r + 2][k]);
            int iy8 = (a[r + 2][k] + 2 * a[r + 2][k + 1] + a[r + 2][k + 2]) - (a[r][k] + 2 * a[r][k + 1] + a[r][k + 2]);
            if ((flipx >> k) & 1u) ix8 = -ix8;
            if (yflip) iy8 = -iy8;
            o[k] = pack_deriv(ix8, iy8, (int)((wb >> (8 * k)) & 0xFFu) - a[r + 1][k + 1]);
        }
        lc[r] = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

// ------------------------------------------------------------------------------------------
// What k_jacobi_strip and k_jacobi_fold share: everything around the sweep.  A kernel family owns its row mapping (which
// image row a register row holds, handed to the helpers below as a callable), its exchange of edge rows and its sweep;
// the strip kernel owns the persistent phases as well.
// ------------------------------------------------------------------------------------------

// Workgroup -> tile (XCD-contiguous), the slot of pairs it belongs to and that slot's pair, the tile's place in the
// pair's grid.  LISTED: the launch may carry a pair list (StripGeom::pair_list); SCALAR: the pair is kept in a scalar register.
struct TileId { int tile, slot, pair, bx, by; };
template <bool LISTED, bool SCALAR>
__device__ __forceinline__ TileId tile_decode(const StripGeom &g)
{
    const int tpp = g.tiles_x * g.tiles_y;
    const int tile = xcd_contiguous_tile(blockIdx.x, gridDim.x);
    const int slot = tile / tpp;
    const int t2 = tile - slot * tpp;
    int pair = slot;
    if constexpr (LISTED) {
        if (g.pair_list) pair = g.pair_list[slot];
    }
    if constexpr (SCALAR) pair = __builtin_amdgcn_readfirstlane(pair);
    const int by = t2 / g.tiles_x, bx = t2 - by * g.tiles_x;
    return TileId{tile, slot, pair, bx, by};
}

// Core membership (for the stores and for Eps) and the trapezoid.  j: row of the region, y: its image row; xl: the lane's
// first column within the region, x0: its image column; T, CH, H: StripGeom's.
// (The forms are what the register allocator of the R = 4 / 5 kernels tolerates.  row_in_core: the rule is the macro, and
// a change to it is one edit; its uses are strip_body (two) and fold_body.  As the condition of the caller's `if` it
// compiles like the parent's code everywhere but in the strip kernel's DERIV launches, where the R = 5 kernels gain a
// spill: those, and only those, take it as the function's value.  (The value everywhere else costs
// k_jacobi_strip<5, 1024, 0, 0> two branches per sweep and moves 30 of the 36 k_jacobi_fold_deriv kernels by 1 - 8
// registers.)  row_dist takes the numbers: with the geometry by reference the same R = 5 _deriv kernels gain a spill.)
#define HS_ROW_IN_CORE(j, y, T, CH, H) ((j) >= (T) && (j) < (T) + (CH) && (y) >= 0 && (y) < (H))
__device__ __forceinline__ bool row_in_core(const int j, const int y, const int T, const int CH, const int H)
{
    return HS_ROW_IN_CORE(j, y, T, CH, H);
}
__device__ __forceinline__ int row_dist(const int j, const int T, const int CH) // distance from the core rows (0 inside)
{
    return j < T ? T - j : (j >= T + CH ? j - (T + CH - 1) : 0);
}
__device__ __forceinline__ bool lane_in_core(const int x0, const int xl, const StripGeom &g)
{
    return (x0 >= 0) && (x0 < g.W) && (xl >= g.HX) && (xl < g.HX + g.CW);
}

// Where does a lane read its four columns x0 .. x0+3?  Inside the image: at x0.  A group that lies completely outside the
// image on the left mirrors onto an aligned group read backwards (columns -1-k <-> k); the same holds on the right when
// W % 4 == 0: those lanes keep the 16-byte loads (from the mirrored address xg, components reversed afterwards: rev).
// Only groups that straddle column W-1 or sit right of it when W % 4 != 0 (and images narrower than the halo) need four
// reflected scalar loads per plane (slow).  side: the region sticks out of the image (workgroup-uniform), inside: the
// group lies wholly inside the image; only a group outside -- side && !inside -- is anything but plain.
// (Two flags in, not their conjunction, and ints out: the conjunction as a value costs k_jacobi_strip<5, 1024, 3, 0> a
// spill, and a struct of 8 bytes is returned as one word, out of which bool flags come as lane values, not as masks.)
__device__ __forceinline__ bool group_inside(const int x0, const int W) { return (x0 >= 0) && (x0 + 3 < W); }
struct ColRule { int xg, rev, slow; };
__device__ __forceinline__ ColRule column_rule(const int x0, const int W, const bool side, const bool inside)
{
    ColRule c{x0, 0, 0};
    if (side && !inside) {
        if (x0 < 0 && -x0 <= W) { c.xg = -x0 - 4; c.rev = 1; }
        else if (x0 >= W && (W & 3) == 0 && 2 * W - x0 - 4 >= 0) { c.xg = 2 * W - x0 - 4; c.rev = 1; }
        else { c.xg = 0; c.slow = 1; }
    }
    return c;
}

// One row of a lane as loaded -> as swept: the pixels p0..p3 go into the register pairs P = (p0, p3), Q = (p1, p2)
// (cross_rows); the packed derivative word becomes the three coefficients of the update (sweep_coefs: one v_rsq per
// pixel), the constant term at the first sweep's scale (scaled state, file header).
__device__ __forceinline__ void unpack(const float4 u, const float4 v, const uint4 cw, const float ilambda,
                                       f2 &uP, f2 &uQ, f2 &vP, f2 &vQ, RowCoef &c)
{
    constexpr int iPx = 0, iPy = 3, iQx = 1, iQy = 2;
    const float lu4[4] = {u.x, u.y, u.z, u.w}, lv4[4] = {v.x, v.y, v.z, v.w};
    uP = f2{lu4[iPx], lu4[iPy]}; uQ = f2{lu4[iQx], lu4[iQy]};
    vP = f2{lv4[iPx], lv4[iPy]}; vQ = f2{lv4[iQx], lv4[iQy]};
    float al[4], be[4], ga[4];
    const uint32_t cc[4] = {cw.x, cw.y, cw.z, cw.w};
#pragma unroll
    for (int p = 0; p < 4; p++) sweep_coefs(cc[p], ilambda, al[p], be[p], ga[p]);
    c.alP = f2{al[iPx], al[iPy]}; c.alQ = f2{al[iQx], al[iQy]};
    c.beP = f2{be[iPx], be[iPy]}; c.beQ = f2{be[iQx], be[iQy]};
    c.gaP = f2{ga[iPx], ga[iPy]} * 4.0f; c.gaQ = f2{ga[iQx], ga[iQy]} * 4.0f;
}

// The load phase (HS_LOAD_PHASE, below, is what the kernels call): load_rows, then (!DERIV) unpack row by row, then
// for a side tile (workgroup-uniform: the region sticks out of the image on the left or right; the vast majority of
// tiles do not and load with plain aligned 16-byte accesses only) HS_MIRROR_ROW and load_rows_slow.
// load_rows: a lane's R rows of flow and coefficients as loaded, from image rows image_row(r) (reflected here) at column xg
// (column_rule).  ALL rows' loads are issued first and unconditionally -- side tiles then load as fast as interior ones
// (with a branch per row their loads did not overlap: +5 000 cycles per launch on the two edge tile columns, which every
// launch then waited for); zero_in: u_in = v_in = one row of zeros (StripGeom), because under a branch per row the
// compiler waits for each row's two loads before it issues the next row's.  The launch with the derivative pass (DERIV)
// is nearly always the one that starts from zero flow: it reads no flow then and goes straight to the frames
// (strip_derive); otherwise ONE branch around all the rows' loads.
// The rows are unpacked as they arrive, straight behind the loads with no branch in between (a third of the launch's
// set-up is this arithmetic: behind the side tiles' fix-ups the compiler waits for ALL loads first).  So a mirrored
// group is fixed after unpacking (HS_MIRROR_ROW).
template <int R, bool DERIV, class RowOf>
__device__ __forceinline__ void load_rows(const uint32_t *coef, const float *u_in, const float *v_in, const StripGeom &g,
                                          const long long base, const int xg, const RowOf image_row,
                                          float4 (&lu)[R], float4 (&lv)[R], uint4 (&lc)[R])
{
#pragma unroll
    for (int r = 0; r < R; r++) {
        const long long off = base + (long long)mirror_index(image_row(r), g.H) * g.P + xg;
        const long long off_uv = g.zero_in ? (long long)xg : off;
        lc[r] = make_uint4(0u, 0u, 0u, 0u);
        if constexpr (!DERIV) {
            lu[r] = *(const float4 *)(u_in + off_uv);
            lv[r] = *(const float4 *)(v_in + off_uv);
            lc[r] = *(const uint4 *)(coef + off);
        } else {
            lu[r] = lv[r] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    if constexpr (DERIV) {
        if (!g.zero_in) {
#pragma unroll
            for (int r = 0; r < R; r++) {
                const long long off = base + (long long)mirror_index(image_row(r), g.H) * g.P + xg;
                lu[r] = *(const float4 *)(u_in + off);
                lv[r] = *(const float4 *)(v_in + off);
            }
        }
    }
}

// The slow lanes of a side tile (column_rule) fetch their rows as four reflected scalars per plane, and unpack them (!DERIV).
// Wave-uniform: rare (W % 4 != 0, or an image narrower than the halo).
template <int R, bool DERIV, class RowOf>
__device__ __forceinline__ void load_rows_slow(const uint32_t *coef, const float *u_in, const float *v_in, const StripGeom &g,
                                               const float ilambda, const long long base, const int x0, const bool slow,
                                               const RowOf image_row, float4 (&lu)[R], float4 (&lv)[R], uint4 (&lc)[R],
                                               f2 (&uP)[R], f2 (&uQ)[R], f2 (&vP)[R], f2 (&vQ)[R], RowCoef (&cf)[R])
{
    if (__builtin_amdgcn_ballot_w64(slow) != 0) {
        if (slow) {
            const int xa = mirror_index(x0, g.W), xb = mirror_index(x0 + 1, g.W),
                      xc = mirror_index(x0 + 2, g.W), xd = mirror_index(x0 + 3, g.W);
#pragma unroll
            for (int r = 0; r < R; r++) {
                const long long row = base + (long long)mirror_index(image_row(r), g.H) * g.P;
                {
                    const float *uv = u_in + (g.zero_in ? 0 : row), *vv = v_in + (g.zero_in ? 0 : row);
                    lu[r] = make_float4(uv[xa], uv[xb], uv[xc], uv[xd]);
                    lv[r] = make_float4(vv[xa], vv[xb], vv[xc], vv[xd]);
                }
                if constexpr (!DERIV) {
                    const uint32_t *cv = coef + row;
                    lc[r] = make_uint4(cv[xa], cv[xb], cv[xc], cv[xd]);
                    unpack(lu[r], lv[r], lc[r], ilambda, uP[r], uQ[r], vP[r], vQ[r], cf[r]);
                }
            }
        }
    }
}

// A mirrored group (column_rule: rev) arrives reversed: (p0, p1, p2, p3) -> (p3, p2, p1, p0).  Unpacked (!DERIV) that is a
// swap of the halves of every register pair; a DERIV launch has not unpacked yet (the derivative words come in lane order
// from strip_derive) and turns the flow as loaded.
// (A macro on purpose: the R = 4 folded and R = 5 strip kernels sit on the register limit, and with these selects in a
// function of their own -- by reference, by value, per row or for all rows -- the allocator ends up elsewhere: 14 of the 32
// k_jacobi_fold kernels with R <= 4 change registers or spills, k_jacobi_fold<4, 1024, 2, 1> from 5 to 10 spills.)
#define HS_MIRROR_ROW(DERIV, rev, lu, lv, uP, uQ, vP, vQ, cf)                                      \
    do {                                                                                           \
        if constexpr (DERIV) {                                                                     \
            if (rev) {                                                                             \
                lu = make_float4(lu.w, lu.z, lu.y, lu.x);                                          \
                lv = make_float4(lv.w, lv.z, lv.y, lv.x);                                          \
            }                                                                                      \
        } else {                                                                                   \
            uP = rev ? f2_swap(uP) : uP; uQ = rev ? f2_swap(uQ) : uQ;                              \
            vP = rev ? f2_swap(vP) : vP; vQ = rev ? f2_swap(vQ) : vQ;                              \
            cf.alP = rev ? f2_swap(cf.alP) : cf.alP; cf.alQ = rev ? f2_swap(cf.alQ) : cf.alQ;      \
            cf.beP = rev ? f2_swap(cf.beP) : cf.beP; cf.beQ = rev ? f2_swap(cf.beQ) : cf.beQ;      \
            cf.gaP = rev ? f2_swap(cf.gaP) : cf.gaP; cf.gaQ = rev ? f2_swap(cf.gaQ) : cf.gaQ;      \
        }                                                                                          \
    } while (0)

// The load phase as both kernels run it: the steps above in their one order.  side: the region sticks out of the image
// (workgroup-uniform), inside: this lane's group lies in the image; lu, lv, lc: the rows as loaded (float4 / uint4 [R]),
// uP .. cf: the rows as swept.  Taken from the kernel body by name: its arguments coef, u_in, v_in, g and ilambda.
// (A macro for the reason given at HS_MIRROR_ROW: the steps must meet in the kernel's body.)
#define HS_LOAD_PHASE(R, DERIV, side, inside, x0, base, image_row, lu, lv, lc, uP, uQ, vP, vQ, cf)                     \
    do {                                                                                                               \
        const ColRule col_ = column_rule(x0, g.W, side, inside);                                                       \
        const bool mirrored_ = col_.rev != 0;                                                                          \
        load_rows<R, DERIV>(coef, u_in, v_in, g, base, col_.xg, image_row, lu, lv, lc);                                \
        if constexpr (!DERIV) {                                                                                        \
            _Pragma("unroll") for (int r = 0; r < R; r++)                                                              \
                unpack(lu[r], lv[r], lc[r], ilambda, uP[r], uQ[r], vP[r], vQ[r], cf[r]);                               \
        }                                                                                                              \
        if (side) {                                                                                                    \
            _Pragma("unroll") for (int r = 0; r < R; r++)                                                              \
                HS_MIRROR_ROW(DERIV, mirrored_, lu[r], lv[r], uP[r], uQ[r], vP[r], vQ[r], cf[r]);                      \
            load_rows_slow<R, DERIV>(coef, u_in, v_in, g, ilambda, base, x0, col_.slow != 0, image_row, lu, lv, lc,    \
                                     uP, uQ, vP, vQ, cf);                                                              \
        }                                                                                                              \
    } while (0)

// A DERIV launch leaves the complete derivative plane behind: the cores tile the image.
template <int R, class RowOf>
__device__ __forceinline__ void store_deriv_rows(uint32_t *coef_w, const StripGeom &g, const long long base,
                                                 const int x0, const unsigned rowcore, const RowOf image_row, const uint4 (&lc)[R])
{
#pragma unroll
    for (int r = 0; r < R; r++)
        if ((rowcore >> r) & 1u) *(uint4 *)(coef_w + base + (long long)image_row(r) * g.P + x0) = lc[r];
}

// The launch's result: a core lane's core rows, back at scale 1 (exact).
// (non-temporal and agent-scope write-through stores were tried here: both slower)
template <int R, class RowOf>
__device__ __forceinline__ void store_flow_rows(float *u_out, float *v_out, const StripGeom &g,
                                                const long long base, const int x0, const unsigned rowcore, const RowOf image_row,
                                                const f2 (&uP)[R], const f2 (&uQ)[R], const f2 (&vP)[R], const f2 (&vQ)[R])
{
#pragma unroll
    for (int r = 0; r < R; r++) {
        if ((rowcore >> r) & 1u) {
            const long long off = base + (long long)image_row(r) * g.P + x0;
            const float fin = __builtin_ldexpf(1.0f, -2 * g.T);
            // P = (p0, p3), Q = (p1, p2)
            *(float4 *)(u_out + off) = make_float4(uP[r].x * fin, uQ[r].x * fin, uQ[r].y * fin, uP[r].y * fin);
            *(float4 *)(v_out + off) = make_float4(vP[r].x * fin, vQ[r].x * fin, vQ[r].y * fin, vP[r].y * fin);
        }
    }
}

// The diagnostic stamps of a workgroup (its thread 0, stamps != NULL only); returns the closing stamp.
__device__ __forceinline__ unsigned long long store_stamps(unsigned long long *stamps, const unsigned long long st0,
                                                           const unsigned long long sr0, const unsigned long long st1,
                                                           const unsigned long long st2, const int tile)
{
    __builtin_amdgcn_s_waitcnt(0); // stores issued and acknowledged
    unsigned long long *o = stamps + (size_t)blockIdx.x * 8;
    o[0] = st0; o[1] = st1; o[2] = st2;
    const unsigned long long st3 = __builtin_amdgcn_s_memtime();
    o[3] = st3;
    o[4] = sr0; o[5] = __builtin_amdgcn_s_memrealtime();
    o[6] = (unsigned long long)__builtin_amdgcn_s_getreg(((4 - 1) << 11) | (0 << 6) | 20); // XCC_ID
    o[7] = (unsigned long long)tile;
    return st3;
}

// Eps, the workgroup's part.  eps_lds: 32 floats behind the exchange buffers.  lane_id: the lane number as a callable (the
// strip kernel's Eps forms read it from the hardware at every use, see there).
// Wavefront 0 folds up to 16 per-wavefront values and stores the maximum as one word.
template <class Lane>
__device__ __forceinline__ void eps_put_max(const float *vals, const int NW, const Lane lane_id, unsigned *word)
{
    float x = lane_id() < NW ? vals[lane_id()] : 0.f;
    x = wave_max_nonneg(x);
    if (lane_id() == 0) *word = __float_as_uint(x);
}
// Behind a measured sweep s: e = the lane's max |new - old| over its core pixels, at the sweep's scale (4^(s+1): scaled
// state).  EPS == 1: the per-wavefront maximum goes to LDS and wavefront 0 folds the PREVIOUS sweep's values into
// eps_out[(s-1) * eps_stride + workgroup] (so the sweep's one barrier orders both); EPS == 3: the one measured sweep,
// folded after the loop (eps_tail).  lane: the lane number as an expression (evaluated at every use).
// (A macro: this sits inside the sweep loop, and as a function the offsets (s & 1) * 16 and ((s - 1) & 1) * 16 are formed
// apart from the sweep's own s & 1 -- two to three scalar instructions more per sweep in every k_jacobi_strip<R, ., 1, .>.)
#define HS_EPS_FOLD_SWEEP(EPS, e, s, w, NW, lane, eps_lds, eps_out, eps_stride)                                        \
    do {                                                                                                               \
        const float unscale_ = __builtin_ldexpf(1.0f, -2 * ((s) + 1));                                                 \
        if (EPS == 3) {                                                                                                \
            const float e_ = wave_max_nonneg(e) * unscale_;                                                            \
            if ((lane) == 0) eps_lds[16 + (w)] = e_;                                                                   \
        }                                                                                                              \
        if (EPS == 1) {                                                                                                \
            const float e_ = wave_max_nonneg(e) * unscale_;                                                            \
            if ((lane) == 0) eps_lds[((s) & 1) * 16 + (w)] = e_;                                                       \
            if ((s) > 0 && (w) == 0) {                                                                                 \
                float x_ = (lane) < (NW) ? eps_lds[(((s) - 1) & 1) * 16 + (lane)] : 0.f;                               \
                x_ = wave_max_nonneg(x_);                                                                              \
                if ((lane) == 0) eps_out[(size_t)((s) - 1) * (eps_stride) + blockIdx.x] = __float_as_uint(x_);         \
            }                                                                                                          \
        }                                                                                                              \
    } while (0)
// Behind the T sweeps.  EPS == 1: the last sweep's fold.  EPS == 2 / 3: the witness word wit_out[workgroup] = +inf if
// the wavefronts vouch for every sweep that ran in witness mode -- seen_n of them each -- and for EPS == 3 the exact
// second word, Eps of the last sweep.  COUNTS (the strip kernel): the wavefronts hand in their counts; where they took
// turns (wit_sum) the counts add up to that number, otherwise one wavefront must have all.  !COUNTS (the folded kernel,
// where every wavefront looks in every sweep): each hands in its own verdict.
template <int EPS, bool COUNTS, class Lane>
__device__ __forceinline__ void eps_tail(const int T, const int seen_n, const bool wit_sum, const int w, const int NW, const Lane lane_id,
                                         float *eps_lds, unsigned *eps_out, unsigned *wit_out, const int eps_stride)
{
    if (EPS == 1) {
        __syncthreads();
        if (w == 0) eps_put_max(eps_lds + ((T - 1) & 1) * 16, NW, lane_id, eps_out + (size_t)(T - 1) * eps_stride + blockIdx.x);
    }
    if (EPS == 2 || EPS == 3) {
        const int witnessed = EPS == 3 ? T - 1 : T;
        if (lane_id() == 0) eps_lds[w] = COUNTS ? (float)seen_n : (seen_n == witnessed ? __builtin_inff() : 0.f);
        __syncthreads();
        if (w == 0) {
            const float x = lane_id() < NW ? eps_lds[lane_id()] : 0.f;
            const float n = wit_sum ? wave_sum16(x) : wave_max_nonneg(x);
            if (lane_id() == 0) wit_out[blockIdx.x] = __float_as_uint(!COUNTS ? n : n == (float)witnessed ? __builtin_inff() : 0.f);
            if (EPS == 3) eps_put_max(eps_lds + 16, NW, lane_id, eps_out + (size_t)eps_stride + blockIdx.x);
        }
    }
}

// The T sweeps of a launch (or phase).  sweep(s, tag): sweep s in the Eps mode the tag names -- the launch's own (EPS 0, 1,
// 2), or for EPS == 3 witness (2) in all sweeps but the last and measured (1) in the last: a second copy of the sweep code
// after the loop, so that the loop keeps the registers of the witness kernel.  The last sweep is peeled off in the other
// forms too (file header) except EPS == 1; TWO: two sweeps per loop trip (the folded kernel).  (T by reference: the
// strip kernel's sweep reads the same variable, the phase's count; by value the R = 5 derivative kernels take a register more.)
// MARK_LAST: the tag of the copy behind the loop carries kSweepLast on top of its Eps mode, and a sweep that asks for the mark
// reads its Eps mode as the tag masked with kSweepLast - 1 -- so no Eps mode may reach 16.  (Only the strip kernel asks: its
// sweep keeps the interior cross sums apart in the loop's copy alone, a matter of its register allocation.)
constexpr int kSweepLast = 16;
template <int EPS, bool TWO, bool MARK_LAST = false, class Sweep>
__device__ __forceinline__ void run_sweeps(const int &T, const Sweep &sweep)
{
    constexpr int kLast = MARK_LAST ? kSweepLast : 0; // (the strip kernel's sweep wants to know which copy it is)
    if constexpr (EPS == 3) {
#pragma unroll 1
        for (int s = 0; s + 1 < T; s++) sweep(s, std::integral_constant<int, 2>{});
        sweep(T - 1, std::integral_constant<int, 1 + kLast>{});
    } else if constexpr (EPS != 1) {
        int s = 0;
        if constexpr (TWO) {
#pragma unroll 1
            for (; s + 2 < T; s += 2) {
                sweep(s, std::integral_constant<int, EPS>{});
                sweep(s + 1, std::integral_constant<int, EPS>{});
            }
        }
#pragma unroll 1
        for (; s + 1 < T; s++) sweep(s, std::integral_constant<int, EPS>{});
        sweep(T - 1, std::integral_constant<int, EPS + kLast>{});
    } else {
        const int n = T; // (a copy: against the reference the every-sweep strip loops come out 2 blocks and 2 branches larger)
#pragma unroll 1
        for (int s = 0; s < n; s++) sweep(s, std::integral_constant<int, EPS>{});
    }
}

template <int R, int NTMAX, int EPS, int E0, bool DERIV, bool PERSIST = false>
__device__ __forceinline__ void strip_body(const uint32_t *__restrict__ coef,
                                                        const float *__restrict__ u_in,
                                                        const float *__restrict__ v_in,
                                                        float *__restrict__ u_out,
                                                        float *__restrict__ v_out, const StripGeom g,
                                                        const float ilambda,
                                                        unsigned *__restrict__ eps_out, const int eps_stride,
                                                        unsigned long long *__restrict__ stamps,
                                                        const float eps_thr, const uint8_t *__restrict__ fA,
                                                        const uint8_t *__restrict__ fB, uint32_t *__restrict__ coef_w,
                                                        const FrameSrc fs, const PersistArgs pa = PersistArgs())
{
    static_assert(!PERSIST || EPS == 0 || EPS == 2, "the persistent form runs plain or witness phases");
    // EPS == 1: eps_out[sweep * eps_stride + workgroup] receives that workgroup's max |new - old| over
    // its core pixels (plain stores, no atomics; the host reduces over the workgroups afterwards).
    // EPS == 2 ("witness"): the cheap way to PROVE that no sweep of this launch had Eps < epsilon.
    // At the end of a sweep a wavefront whose first row is a core row asks "did u change by >= eps_thr
    // at column x0 of any lane of that row?" -- old and new value come back from the two exchange
    // buffers, so nothing is kept in registers for it -- and counts the
    // per-sweep answers in an SGPR.  Each |change| is a lower bound of that sweep's Eps, so a
    // wavefront that answered yes in EVERY sweep proves Eps_k >= eps_thr for all k of the launch;
    // eps_out[workgroup] = +inf if any wavefront of the workgroup did, else 0.
    // EPS == 3: witness for sweeps 0 .. T-2 (word eps_out[workgroup]) and the exact Eps of the LAST sweep
    // (word eps_out[eps_stride + workgroup]): what the final launch of an ITER|EPS solve needs -- "no early
    // stop before the budget" plus last_eps -- at the price of one measured sweep instead of T.
    // `stamps` is a diagnostic buffer (NULL in production: no stamp executes).  When set, lane 0 of
    // wavefront 0 records shader-clock / 100 MHz wall-clock stamps at the phase boundaries into
    // memory nothing else reads (HSFLOW_DEBUG_STAMPS, see hs_runtime.hip.h).
    extern __shared__ __attribute__((aligned(16))) float4 ex[]; // [2][NW][4][64], then 32 floats for Eps
    unsigned long long st0 = 0, sr0 = 0, st1 = 0, st2 = 0;
    if (stamps) { st0 = __builtin_amdgcn_s_memtime(); sr0 = __builtin_amdgcn_s_memrealtime(); }
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int NW = g.NW;
    float *eps_lds = (float *)(ex + (size_t)2 * NW * 4 * 64);
    // Synchronisation between sweeps: ONE workgroup barrier per sweep.  (Tried and measured slower, 0.220 vs 0.200 ms
    // at 1080p / 100 sweeps in round 1: per-wavefront counters in LDS, each wavefront waiting only for the strips
    // directly above and below.)
    const TileId tl = tile_decode<!PERSIST, false>(g); // (the persistent launch always works on every pair: no list, and not a scalar register for one)
    const int x0 = tl.bx * g.CW - g.HX + 4 * lane;
    const int y0 = tl.by * g.CH - g.T + w * R;
    const long long base = (long long)tl.pair * g.plane;
    const bool xin = group_inside(x0, g.W);
    // The sweep code is written for ONE checkerboard phase: pixel p0 of register row 0 must be an "E0" pixel
    // (x0 % 4 == 0, so that is the parity of the row, counted from the frame's row 0: g.org).  R even: every strip
    // of the launch starts on a row of the parity of T + org (CH is even), which is the template parameter E0 -- the
    // host launches the matching kernel.
    // R odd: strips alternate, E0 = 0 is the only instantiation, and a strip that starts on an odd row keeps its
    // rows in REVERSE order (register row r = image row y0 + R-1-r): mirrored in y, an odd pixel forms the pair
    // sums of an even one (update_cv: U and D swap roles), so the same code computes the same bits.  Only the
    // addressing knows: which image row a register row is, and which exchange slot holds a neighbour's edge row.
    const bool rev = (R & 1) != 0 && ((y0 + g.org) & 1) != 0; // wave-uniform
    auto img_row = [&](int r) { return rev ? R - 1 - r : r; }; // row of the strip that register row r holds
    auto image_row = [&](int r) { return y0 + img_row(r); };

    f2 uP[R], uQ[R], vP[R], vQ[R];
    RowCoef cf[R];
    float4 lu[R], lv[R];
    uint4 lc[R];
    const int rx0 = tl.bx * g.CW - g.HX;
    const bool xedge = !(rx0 >= 0 && rx0 + 256 <= g.W); // workgroup-uniform: the region sticks out of the image on the left or right
    HS_LOAD_PHASE(R, DERIV, xedge, xin, x0, base, image_row, lu, lv, lc, uP, uQ, vP, vQ, cf);
    // core membership (for the stores and for Eps): rows as a bit mask, lanes as a flag
    unsigned rowcore = 0;
    int rdist[R]; // distance of each row from the core rows: wave-uniform
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int j = w * R + img_row(r);
        const int y = image_row(r);
        if constexpr (DERIV) {
            if (row_in_core(j, y, g.T, g.CH, g.H)) rowcore |= 1u << r;
        } else {
            if (HS_ROW_IN_CORE(j, y, g.T, g.CH, g.H)) rowcore |= 1u << r;
        }
        rdist[r] = row_dist(j, g.T, g.CH);
    }
    const bool lanecore = lane_in_core(x0, 4 * lane, g);
    if constexpr (DERIV) {
        const unsigned keep = (fs.keepA != nullptr && lanecore) ? rowcore : 0u; // the core rows of a core lane
        strip_derive<R, true>(fA, fB, g, base, x0, rev ? y0 + R - 1 : y0, rev ? -1 : 1, xin, lc, fs, keep);
#pragma unroll
        for (int r = 0; r < R; r++) unpack(lu[r], lv[r], lc[r], ilambda, uP[r], uQ[r], vP[r], vQ[r], cf[r]);
    }
    const int pr = g.W - 1 - x0; // image columns of this group: 0..min(pr,3)
    // From here on the Eps / witness kernels read the lane number from the hardware where it is used (hs_lane_now): nothing
    // below keeps it in a register, and with the three LDS addresses of a sweep formed from that one value the witness kernel
    // no longer spills (it reloaded a coefficient pair in every sweep: ITER|EPS stream 0.1325 -> 0.1254 ms per pair).  The
    // plain kernel has the registers and is 0.8 % faster with the lane number kept.
    constexpr bool LANE_HW = EPS != 0 || PERSIST;
    const auto lane_id = [&]() __attribute__((always_inline)) { return LANE_HW ? hs_lane_now() : lane; };
    unsigned epscore = 0; // the core rows that lie in the Eps window (wave-uniform; all of them unless hsflow_set_eps_rows narrowed it)
    if (EPS != 0) {
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int y = image_row(r);
            if (((rowcore >> r) & 1u) && y >= g.ey0 && y < g.ey1) epscore |= 1u << r;
        }
    }
    if (DERIV && lanecore) store_deriv_rows<R>(coef_w, g, base, x0, rowcore, image_row, lc);

    // One row: neighbour sums from the cross sums of its two boundaries (sc below, sp above), update in place.
    // A row at distance d from the core is only needed through sweep T-1-d (trapezoid): later sweeps skip it
    // (wave-uniform branch), which trims the redundant halo work by about half.  PE = parity of the row's pixel p0.
    // The guards read ONE scalar per sweep: bit r of `act` = register row r is still swept, bit r of `actb` = row r or
    // row r + 1 is (the boundary between them is needed).  The rows of a strip that are still swept are an interval of
    // its image rows, i = n0 + s .. R-1 - (m0 + s) (n0, m0 below: from the strip's place in the region; a strip of core
    // rows has both far below zero and never loses a row), so the mask is two 64-bit tables of ones shifted by s and met
    // in one word -- no compare per row.  The optimiser must not see through it (it turns the bits back into
    // one compare and branch per row and boundary): the mask passes through an empty asm, as the lane number does.
#define HS_LIKELY(c) (PERSIST ? !!(c) : __builtin_expect(!!(c), 1))
#define HS_ACT(r) HS_LIKELY(((act >> (r)) & 1u) != 0u)
#define HS_ROW(r, PE, SC, SP)                                                                      \
    do {                                                                                           \
        if (HS_LIKELY(((actr >> (r)) & 1u) != 0u)) {                                               \
            f2 ouP, ouQ, ovP, ovQ;                                                                 \
            if (EM == 1) { ouP = uP[r]; ouQ = uQ[r]; ovP = vP[r]; ovQ = vQ[r]; }                   \
            if (HS_DIAG & 8) uP[r] += SC.uP + SP.uP;                                               \
            else strip_row_update<PE>(uP[r], uQ[r], vP[r], vQ[r], SC, SP, cf[r]);                  \
            if (EM == 1) {                                                                         \
                if ((epscore >> (r)) & 1u) { /* wave-uniform; lanes outside the core are masked once per sweep */ \
                    const f2 dUP = sweep_diff(ouP, uP[r]), dUQ = sweep_diff(ouQ, uQ[r]), dVP = sweep_diff(ovP, vP[r]), dVQ = sweep_diff(ovQ, vQ[r]); \
                    if (HS_LIKELY(!xedge)) { /* workgroup-uniform: every column of the region is an image column */ \
                        e = fmaxf(fmaxf(e, fabsf(dUP.x)), fabsf(dUP.y));                           \
                        e = fmaxf(fmaxf(e, fabsf(dUQ.x)), fabsf(dUQ.y));                           \
                        e = fmaxf(fmaxf(e, fabsf(dVP.x)), fabsf(dVP.y));                           \
                        e = fmaxf(fmaxf(e, fabsf(dVQ.x)), fabsf(dVQ.y));                           \
                    } else {                                                                       \
                        /* image columns of the group are p0 .. p(pr); P = (p0, p3), Q = (p1, p2) */ \
                        e = fmaxf(e, fmaxf(fabsf(dUP.x), fabsf(dVP.x)));                           \
                        if (pr >= 1) e = fmaxf(e, fmaxf(fabsf(dUQ.x), fabsf(dVQ.x)));              \
                        if (pr >= 2) e = fmaxf(e, fmaxf(fabsf(dUQ.y), fabsf(dVQ.y)));              \
                        if (pr >= 3) e = fmaxf(e, fmaxf(fabsf(dUP.y), fabsf(dVP.y)));              \
                    }                                                                              \
                }                                                                                  \
            }                                                                                      \
        }                                                                                          \
    } while (0)
    // cross sums of the boundary below register row A (row B underneath), needed while either row is still swept
#define HS_CROSS(S, PE, A, B)                                                                      \
    do {                                                                                           \
        if (HS_LIKELY(((actb >> (A)) & 1u) != 0u)) { /* B is A + 1 */                              \
            if (HS_DIAG & 8) S.uP = uP[A] + uP[B];                                                 \
            else cross_rows<PE>(S, uP[A], uQ[A], vP[A], vQ[A], uP[B], uQ[B], vP[B], vQ[B]);        \
        }                                                                                          \
    } while (0)
#define HS_PUBLISH(buf, ln)                                                                         \
    do {                                                                                           \
        float4 *exw = ex + ((size_t)((buf) * NW + w) * 4) * 64 + (ln);                             \
        exw[0] = make_float4(uP[0].x, uP[0].y, uQ[0].x, uQ[0].y);                                  \
        exw[64] = make_float4(vP[0].x, vP[0].y, vQ[0].x, vQ[0].y);                                 \
        exw[128] = make_float4(uP[R - 1].x, uP[R - 1].y, uQ[R - 1].x, uQ[R - 1].y);                \
        exw[192] = make_float4(vP[R - 1].x, vP[R - 1].y, vQ[R - 1].x, vQ[R - 1].y);                \
    } while (0)

    // Exchange slots: ex[buf][wave][0..3][lane] = {register row 0: u, v; register row R-1: u, v}.
    // Sweep s reads buffer s&1 and publishes its new edge rows into buffer (s+1)&1, then meets the
    // other wavefronts at ONE barrier.  The edge rows are updated and published FIRST so that the
    // LDS writes drain while the interior rows are being computed.
    if (stamps) st1 = __builtin_amdgcn_s_memtime();
    // Whose slot is the row above register row 0 (wu, su) and the row below register row R-1 (wd, sd)?  A strip's
    // bottom image row is its register row R-1 (slot pair 2) unless it is reversed (then row 0: slot pair 0), its
    // top image row the other one; for odd R the neighbouring strips are reversed exactly when this one is not.
    // A reversed strip has the strip BELOW it above its register row 0.
    // (at the region edge the strip's own edge row stands in: junk the validity argument tolerates)
    const bool nrev = (R & 1) != 0 && !rev; // the strips above and below are reversed
    const int wa = w > 0 ? w - 1 : w, sa = w > 0 ? (nrev ? 0 : 2) : 0;            // image row above this strip
    const int wb = w < NW - 1 ? w + 1 : w, sb = w < NW - 1 ? (nrev ? 2 : 0) : 2;  // image row below this strip
    const int wu = rev ? wb : wa, su = rev ? sb : sa;
    const int wd = rev ? wa : wb, sd = rev ? sa : sb;
    int seen_n = 0; // EPS == 2, wave-uniform: sweeps so far that had a change >= eps_thr (a counter: a
                    // loop-carried flag makes the register allocator spill inside the loop)
    const unsigned long long wit_mask = (epscore & 1u) ? __builtin_amdgcn_ballot_w64(lanecore) : 0ull; // lanes whose answer counts
    // Who looks, and when: the wavefronts whose rows are all core rows take turns, one of them per sweep (a sweep
    // needs ONE witness in the workgroup; sixteen wavefronts looking in every sweep cost 4 % of the launch).  A
    // workgroup without such a wavefront (thin cores, clipped bottom tiles) keeps the old rule: every wavefront whose
    // register row 0 is a core row looks in every sweep.  wit_cnt counts down to this wavefront's next turn.
    const int core_here = min(g.CH, g.H - tl.by * g.CH);
    const int wit_lo = (g.T + R - 1) / R, wit_n = (g.T + core_here) / R - wit_lo; // wavefronts wit_lo .. wit_lo + wit_n - 1
    const bool wit_rot = wit_n > 0;
    const int wit_per = wit_rot ? wit_n : 1;
    const int wit_cnt0 = !wit_rot ? 0 : (w >= wit_lo && w < wit_lo + wit_n) ? w - wit_lo : (1 << 30);
    int wit_cnt = wit_cnt0;
    // Sweeps of the current phase: the launch's T, except in the last phase of a persistent launch (PERSIST).  A shorter
    // phase simply starts further down the trapezoid: rows further than Tp - 1 from the core are never swept.
    int Tp = g.T;
    unsigned long long act_lo = 0, act_hi = 0; // the trapezoid's tables of the current phase (HS_ACT)
    // One sweep.  EM is the Eps mode of THIS sweep: the launch's own (EPS 0, 1, 2), or for EPS == 3 witness
    // (2) in all sweeps but the last and measured (1) in the last -- a second copy of the sweep code after the
    // loop, so that the loop keeps the registers of the witness kernel.  E0 = parity of pixel p0 of register
    // row 0 (image row y0 + image column x0, x0 % 4 == 0): wave-uniform, rows alternate from there.
    // (A second, straight-line copy of the sweep for wavefronts whose rows are all core rows -- no compare and branch per
    // row -- was tried and rejected: two copies of the body make the register allocator spill 66 registers.  So was a
    // trapezoid per WAVEFRONT instead of per row, one branch per sweep: 16 -> 3 branches and 40 -> 12 scalar instructions
    // in the loop, but the straight-line body keeps more values alive and the ITER kernel then spills inside the loop:
    // ITER|EPS 0.1573 -> 0.1556 ms, ITER 0.1522 -> 0.1555 ms at 1080p / 100.)
    auto sweep = [&](const int s, auto em_tag) __attribute__((always_inline)) {
        constexpr int EM = decltype(em_tag)::value & (kSweepLast - 1);
        constexpr bool IN_LOOP = (decltype(em_tag)::value & kSweepLast) == 0; // (not the copy of the sweep behind the loop)
#if HS_DIAG & 4 /* diagnostic build: every row swept in every sweep (no trapezoid) */
        unsigned act = ~0u;
#else
        unsigned act = (unsigned)((act_lo << s) >> 32) & (unsigned)(act_hi >> (24 + s)); // (bits from R on: never looked at)
#endif
        unsigned actb = act | (act >> 1), actr = act; // (actr: the row's own guard, apart from the edge rows' first use of act)
        // (not in the every-sweep kernels, which are off the hot path: at R = 6 they hold the sweep counter in a vector
        // register, and the asm's scalar operand cannot be had from it)
        if constexpr (EPS != 1) asm volatile("" : "+s"(act), "+s"(actb), "+s"(actr));
        // (scaled state: this sweep takes the flow from scale 4^s to 4^(s+1))
        // eps_thr * 4^(s+1) by integer arithmetic on the exponent: scalar instructions only (v_ldexp + v_readfirstlane put
        // a vector-to-scalar round trip into every sweep).  Exact while eps_thr is normal and the product finite; past
        // that the sum reads +inf for one sweep and then carries into the sign bit, where every lane would pass.  The host
        // sends only a threshold that stays exact over all T sweeps (hs_stop_rule.h: never zero, never a denormal, exponent
        // field + 2 T <= 254), and runs no witness launch where there is none.
        const float thr_s = __int_as_float(__float_as_int(eps_thr) + ((s + 1) << 24));
#if HS_DIAG & 1 /* diagnostic build (wrong results): no LDS traffic, the strip's own edge rows stand in */
        const float4 hu4 = make_float4(uP[0].x, uP[0].y, uQ[0].x, uQ[0].y), hv4 = make_float4(vP[0].x, vP[0].y, vQ[0].x, vQ[0].y);
        const float4 du4 = make_float4(uP[R - 1].x, uP[R - 1].y, uQ[R - 1].x, uQ[R - 1].y), dv4 = make_float4(vP[R - 1].x, vP[R - 1].y, vQ[R - 1].x, vQ[R - 1].y);
#else
        // (Eps / witness kernels: the three LDS addresses of a sweep are formed from ONE value, the lane number as the
        // hardware gives it at this point (hs_lane_now): left alone the compiler keeps three loop-invariant address
        // registers alive across the sweep loop, which has none to spare -- the witness kernel then reloaded a spilled
        // coefficient pair in every sweep.)
        const int lane_l = lane_id();
        const float4 *eu = ex + ((size_t)((s & 1) * NW + wu) * 4 + su) * 64 + lane_l;
        const float4 *ed = ex + ((size_t)((s & 1) * NW + wd) * 4 + sd) * 64 + lane_l;
        // (Idle strips -- late sweeps, halo wavefronts -- still read and publish their edge rows.  Gating the reads makes the
        // register allocator spill inside the loop; gating only the publish costs two more branches per sweep than the
        // LDS traffic it saves: 0.1363 against 0.1353 ms per pair, round 3.)
        const float4 hu4 = eu[0], hv4 = eu[64]; // old row above the strip
        const float4 du4 = ed[0], dv4 = ed[64]; // old row below the strip
#endif
        const f2 huP = f2{hu4.x, hu4.y}, huQ = f2{hu4.z, hu4.w}, hvP = f2{hv4.x, hv4.y}, hvQ = f2{hv4.z, hv4.w};
        const f2 duP = f2{du4.x, du4.y}, duQ = f2{du4.z, du4.w}, dvP = f2{dv4.x, dv4.y}, dvQ = f2{dv4.z, dv4.w};

        float e = 0.f;
        constexpr int EL = E0 ^ ((R - 1) & 1); // parity of the last register row
        Cross sA, s0, sK, sL; // above row 0, below row 0, above row R-1, below row R-1
        const bool wturn = EM == 2 && (PERSIST ? wit_cnt == 0 : __builtin_expect(wit_cnt == 0, 0)); // wave-uniform: this wavefront is the sweep's witness
        float w0 = 0.f;
        if (wturn) w0 = uP[0].x; // witness: u at column x0 of register row 0 before the sweep
        // --- first row (the strip's upper edge)
        if (HS_ACT(0)) cross_rows<E0 ^ 1>(sA, huP, huQ, hvP, hvQ, uP[0], uQ[0], vP[0], vQ[0]);
        if (R == 1) {
            if (HS_ACT(0)) cross_rows<E0>(s0, uP[0], uQ[0], vP[0], vQ[0], duP, duQ, dvP, dvQ);
        } else {
            constexpr int R1 = R > 1 ? 1 : 0;
            HS_CROSS(s0, E0, 0, R1);
        }
        HS_ROW(0, E0, s0, sA);
        // witness: did u change by >= eps_thr at column x0 of register row 0 (where that is a core row) in any lane?
        // (The host runs witness launches only with plans in which some wavefront has such a row: strip_has_witness.)
        if (EM == 2) { // (wit_mask: the core lanes if register row 0 is a core row, else none)
            if (wturn) seen_n += (__builtin_amdgcn_ballot_w64(fabsf(sweep_diff(w0, uP[0].x)) >= thr_s) & wit_mask) != 0 ? 1 : 0;
            wit_cnt = wturn ? wit_per - 1 : wit_cnt - 1;
        }
        if (R >= 2) {
            // --- last row (the lower edge), then both edges go to the other wavefronts
            constexpr int RM = R > 2 ? R - 2 : 0;
            if (HS_ACT(R - 1)) cross_rows<EL>(sL, uP[R - 1], uQ[R - 1], vP[R - 1], vQ[R - 1], duP, duQ, dvP, dvQ);
                if (R >= 3) HS_CROSS(sK, EL ^ 1, RM, R - 1);
            if (R == 2) HS_ROW(R - 1, EL, sL, s0);
            else HS_ROW(R - 1, EL, sL, sK);
        }
#if !(HS_DIAG & 1)
        if (s + 1 < Tp) HS_PUBLISH((s + 1) & 1, lane_l);
#endif
        // --- interior rows, top to bottom: each needs the cross sum above it (kept) and the one below (new)
        if (R >= 3) {
            Cross sp = s0;
            // (one object per boundary: a single `sc` declared in the loop body is ONE variable to the optimiser, so the sum of
            // a boundary no longer needed was the previous boundary's, kept alive by four v_mov_b64 ahead of the guard in
            // every sweep of every wavefront; apart, an unneeded sum is simply undefined)
            Cross scs[R], sc1;
#pragma unroll
            for (int r = 1; r < R - 1; r++) {
                Cross &sc = IN_LOOP && EM != 1 ? scs[r] : sc1; // (only where it pays: apart, a measured sweep and the copy behind the loop spill more)
                if (r == R - 2) sc = sK;
                else {
                    const int rn = r + 1 < R ? r + 1 : r;
                    if (r & 1) HS_CROSS(sc, E0 ^ 1, r, rn);
                    else HS_CROSS(sc, E0, r, rn);
                }
                if (r & 1) HS_ROW(r, E0 ^ 1, sc, sp);
                else HS_ROW(r, E0, sc, sp);
                sp = sc;
            }
        }
        if constexpr (EM == 1) HS_EPS_FOLD_SWEEP(EPS, lanecore ? e : 0.f, s, w, NW, lane_id(), eps_lds, eps_out, eps_stride);
#if !(HS_DIAG & 2) /* diagnostic build: no barrier */
        if (s + 1 < Tp) __syncthreads();
#endif
        // diagnostic (stamps != NULL only): when each sweep ended -- all wavefronts leave the barrier together, so
        // wavefront 0 sees the workgroup's sweep times; slots behind the 8 phase stamps of every workgroup
#if HS_SWEEP_STAMPS /* (diagnostic builds: tools/diag_build.sh; tools/stamps_sweeps.py reads them) */
        if (stamps && gridDim.x <= 8192 && threadIdx.x == 0)
            stamps[(size_t)gridDim.x * 8 + (size_t)blockIdx.x * 32 + (s & 31)] = __builtin_amdgcn_s_memtime();
#endif
    };
    // Wavefronts whose rows are all core rows never drop out of a sweep (trapezoid): they are the ones every barrier waits
    // for, so they go first at the issue port (-0.3 % one context, -0.7 % in the stream).
    if (rowcore == (1u << R) - 1u) __builtin_amdgcn_s_setprio(1);
    // PERSIST: the phases of the solve; otherwise one pass (the `break` after the store is unconditional).
    int ph = 0;
    unsigned flag_base = 0; // this tile's phase counter at the start of the launch (all tiles agree; wavefront 0 only)
    unsigned long long pt_sweep = 0, pt_pub = 0, pt_wait = 0, pt_load = 0, pt0 = 0, pt_first = 0; // PERSIST diagnostics (stamps)
    if constexpr (PERSIST) {
        if (w == 0) flag_base = (unsigned)__builtin_amdgcn_readfirstlane((int)load_u32_sc1(pa.flags + tl.tile));
    }
#pragma unroll 1
    for (;;) {
    if constexpr (PERSIST) {
        Tp = ph == pa.n_phase - 1 ? pa.T_last : g.T;
        seen_n = 0;
        wit_cnt = wit_cnt0;
        if (stamps && ph == 0) pt_first = pt0 = __builtin_amdgcn_s_memtime();
    }
    {   // The trapezoid of this phase: row j of the region is swept while T - j <= Tp-1 - s and j - (T + CH - 1) <= Tp-1 - s.
        // Clamped to what the 32 sweeps a launch can have (kMaxFuse) tell apart, so that the tables fit 64 bits (R <= 8).
        static_assert(R <= 8, "the trapezoid tables hold 8 rows per lane");
        const int n0 = min(max(g.T - Tp + 1 - w * R, -32), R), m0 = min(max(w * R + R + 1 - g.T - g.CH - Tp, -32), R);
        act_lo = ~0ull << (32 + (rev ? m0 : n0));     // ones from bit 32 + lo: << s, upper word = the bits r >= lo + s
        act_hi = ~0ull >> (40 - R + (rev ? n0 : m0)); // ones up to bit 24 + R-1 - hi: >> (24 + s) = the bits r <= R-1 - (hi + s)
    }
    HS_PUBLISH(0, lane_id());
    __syncthreads();
    if (PERSIST && stamps && ph > 0) { // (the reloaded rows are first used by the publish above: their latency belongs to the reload)
        const unsigned long long t = __builtin_amdgcn_s_memtime();
        pt_load += t - pt0;
        pt0 = t;
    }
    run_sweeps<EPS, false, true>(Tp, sweep);
    unsigned *const eps_ph = PERSIST ? eps_out + (size_t)ph * eps_stride : eps_out; // PERSIST: one row of words per phase
    eps_tail<EPS, true>(Tp, seen_n, wit_rot, w, NW, lane_id, eps_lds, eps_out, eps_ph, eps_stride);
    if (stamps) st2 = __builtin_amdgcn_s_memtime();

    if constexpr (!PERSIST) {
        // (the lane's column is worked out afresh from a copy of the lane number the optimiser cannot see through: kept
        // alive across the sweep loop it is one of the three registers the loop has no room for -- every spilled register
        // is 250 KB of scratch written and read per launch, which showed up as HBM writes: profiles/r03_traffic_by_kernel.json)
        int lane_s = lane_id();
        if constexpr (!LANE_HW) asm volatile("" : "+v"(lane_s)); // (the kept lane number: a copy the optimiser cannot see through)
        const int x0s = tl.bx * g.CW - g.HX + 4 * lane_s;
        if (lanecore) store_flow_rows<R>(u_out, v_out, g, base, x0s, rowcore, image_row, uP, uQ, vP, vQ);
        break;
    } else {
        if (stamps) { pt_sweep += st2 - pt0; pt0 = st2; }
        // --- publish: the core rows go back to scale 1 in their registers (exact) and out with write-through stores
        const __amdgpu_buffer_rsrc_t pu = plane_rsrc(pa.ub[ph & 1]), pv = plane_rsrc(pa.vb[ph & 1]);
        const float fin = __builtin_ldexpf(1.0f, -2 * Tp);
        // The lane's column and where it reads its halo from are worked out afresh in every phase, from a copy of the
        // lane number the optimiser cannot see through: hoisted out of the phase loop they would be two more registers
        // alive across the sweep loop, which has none to spare (the sweep then reloads spilled coefficients).
        const int lane_x = lane_id();
        const int x0x = tl.bx * g.CW - g.HX + 4 * lane_x;
        // (host: W % 4 == 0 and W >= 256, so no group straddles the border: never slow)
        const ColRule colx = column_rule(x0x, g.W, xedge, group_inside(x0x, g.W));
        const int xgx = colx.xg;
        const bool xrevx = colx.rev != 0;
#pragma unroll
        for (int r = 0; r < R; r++) {
            if ((rowcore >> r) & 1u) { // wave-uniform
                uP[r] *= fin; uQ[r] *= fin; vP[r] *= fin; vQ[r] *= fin;
                if (lanecore) {
                    const unsigned row = 4u * (unsigned)(base + (long long)image_row(r) * g.P); // wave-uniform
                    store_f4_sc1(pu, row, 4u * (unsigned)x0x, f4{uP[r].x, uQ[r].x, uQ[r].y, uP[r].y});
                    store_f4_sc1(pv, row, 4u * (unsigned)x0x, f4{vP[r].x, vQ[r].x, vQ[r].y, vP[r].y});
                }
            }
        }
        if (ph == pa.n_phase - 1) break; // the launch's end publishes the last phase
        // the constant term back to the scale a phase starts with: a row was swept max(0, Tp - rdist) times
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int nact = Tp - rdist[r] > 0 ? Tp - rdist[r] : 0;
            const float back = __builtin_ldexpf(1.0f, -2 * nact);
            cf[r].gaP *= back; cf[r].gaQ *= back;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this wavefront's stores have been written through
        __syncthreads();                                  // ... and so have every other wavefront's
        if (stamps) { const unsigned long long t = __builtin_amdgcn_s_memtime(); pt_pub += t - pt0; pt0 = t; }
        int *const dead_lds = (int *)(eps_lds + 31);
        if (w == 0) {
            const unsigned target = flag_base + (unsigned)ph + 1u; // "phase ph of this tile is published"
            if (lane_id() == 0) __hip_atomic_store(pa.flags + tl.tile, target, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // lanes 0..7 watch the 8 neighbouring tiles (same pair), lane 8 the abort word
            int nb = -1;
            if (lane_id() < 8) {
                const int k = lane_id() < 4 ? lane_id() : lane_id() + 1; // 0..8 without the centre
                const int nx = tl.bx + k % 3 - 1, ny = tl.by + k / 3 - 1;
                if (nx >= 0 && nx < g.tiles_x && ny >= 0 && ny < g.tiles_y) nb = tl.slot * g.tiles_x * g.tiles_y + ny * g.tiles_x + nx;
            } else if (lane_id() == 8) nb = (int)gridDim.x;
            const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
            int dead = 0;
            for (;;) {
                unsigned v = target;
                if (nb >= 0) v = load_u32_sc1(pa.flags + nb);
                const bool aborted = lane_id() == 8 && v != 0u;
                const bool behind = lane_id() < 8 && (int)(v - target) < 0;
                if (__builtin_amdgcn_ballot_w64(aborted) != 0) { dead = 1; break; }
                if (__builtin_amdgcn_ballot_w64(behind) == 0) break;
                if (__builtin_amdgcn_s_memrealtime() - t0 > (unsigned long long)pa.wait_ticks) { // a neighbour never came
                    dead = 1;
                    if (lane_id() == 0) {
                        __hip_atomic_store(pa.flags + gridDim.x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        __hip_atomic_store(pa.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    }
                    break;
                }
                __builtin_amdgcn_s_sleep(4);
            }
            if (lane_id() == 0) *dead_lds = dead;
        }
        __syncthreads();
        if (__builtin_amdgcn_readfirstlane(*dead_lds)) return; // workgroup-uniform (and said so: a divergent exit would put the loop's counters into VGPRs)
        if (stamps) { const unsigned long long t = __builtin_amdgcn_s_memtime(); pt_wait += t - pt0; pt0 = t; }
        // --- reload the halo: whole rows outside the core rows, the side lanes of core rows (host: W % 4 == 0 and
        // the image at least as large as the region, so every group is an aligned group, read backwards where mirrored)
        {
            f4 tu[R], tv[R];
#pragma unroll
            for (int r = 0; r < R; r++) {
                const unsigned row = 4u * (unsigned)(base + (long long)mirror_index(image_row(r), g.H) * g.P); // wave-uniform
                tu[r] = f4{uP[r].x, uQ[r].x, uQ[r].y, uP[r].y};
                tv[r] = f4{vP[r].x, vQ[r].x, vQ[r].y, vP[r].y};
                if (!((rowcore >> r) & 1u) || !lanecore) {
                    tu[r] = load_f4_sc1(pu, row, 4u * (unsigned)xgx);
                    tv[r] = load_f4_sc1(pv, row, 4u * (unsigned)xgx);
                }
            }
#pragma unroll
            for (int r = 0; r < R; r++) {
                if (xrevx) { // (mirrored groups lie outside the image: never core lanes)
                    tu[r] = f4{tu[r].w, tu[r].z, tu[r].y, tu[r].x};
                    tv[r] = f4{tv[r].w, tv[r].z, tv[r].y, tv[r].x};
                }
                uP[r] = f2{tu[r].x, tu[r].w}; uQ[r] = f2{tu[r].y, tu[r].z};
                vP[r] = f2{tv[r].x, tv[r].w}; vQ[r] = f2{tv[r].y, tv[r].z};
            }
        }
        ph++;
    }
    } // phases
#undef HS_ROW
#undef HS_ACT
#undef HS_LIKELY
#undef HS_CROSS
#undef HS_PUBLISH
    if (stamps && threadIdx.x == 0) {
        const unsigned long long st3 = store_stamps(stamps, st0, sr0, st1, st2, tl.tile);
        if (PERSIST && gridDim.x <= 8192) { // totals over the phases: sweeps, publish, wait, reload (cycles)
            unsigned long long *q = stamps + (size_t)gridDim.x * 8 + (size_t)blockIdx.x * 32;
            q[0] = pt_sweep; q[1] = pt_pub; q[2] = pt_wait; q[3] = pt_load; q[4] = pt_first - st1; q[5] = st3 - st2;
        }
    }
}

template <int R, int NTMAX, int EPS, int E0>
__global__ __launch_bounds__(NTMAX) void k_jacobi_strip(const uint32_t *__restrict__ coef,
                                                        const float *__restrict__ u_in,
                                                        const float *__restrict__ v_in,
                                                        float *__restrict__ u_out,
                                                        float *__restrict__ v_out, const StripGeom g,
                                                        const float ilambda,
                                                        unsigned *__restrict__ eps_out, const int eps_stride,
                                                        unsigned long long *__restrict__ stamps,
                                                        const float eps_thr)
{
    strip_body<R, NTMAX, EPS, E0, false>(coef, u_in, v_in, u_out, v_out, g, ilambda, eps_out, eps_stride, stamps, eps_thr,
                                     nullptr, nullptr, nullptr, FrameSrc{0, 0, nullptr, nullptr});
}

// First launch of a solve with the derivative pass folded in: reads the two frames instead of the packed
// derivative plane and writes that plane for the launches that follow (and for hsflow_get_derivatives).
// fs: where the frames lie -- the context's planes, or the caller's, which this launch then also copies (FrameSrc).
template <int R, int NTMAX, int EPS, int E0>
__global__ __launch_bounds__(NTMAX) void k_jacobi_strip_deriv(const uint8_t *__restrict__ fA,
                                                              const uint8_t *__restrict__ fB, const FrameSrc fs,
                                                              uint32_t *__restrict__ coef_w,
                                                              const float *__restrict__ u_in,
                                                              const float *__restrict__ v_in,
                                                              float *__restrict__ u_out,
                                                              float *__restrict__ v_out, const StripGeom g,
                                                              const float ilambda,
                                                              unsigned *__restrict__ eps_out, const int eps_stride,
                                                              unsigned long long *__restrict__ stamps,
                                                              const float eps_thr)
{
    strip_body<R, NTMAX, EPS, E0, true>(nullptr, u_in, v_in, u_out, v_out, g, ilambda, eps_out, eps_stride, stamps, eps_thr,
                                    fA, fB, coef_w, fs);
}

// One launch for the whole solve (PersistArgs above).  DERIV: phase 0 computes the derivative words from the frames and
// leaves the packed plane behind (coef_rw is written); otherwise coef_rw is only read.
template <int R, int NTMAX, int EPS, int E0, bool DERIV>
__global__ __launch_bounds__(NTMAX) void k_jacobi_strip_persist(const uint8_t *__restrict__ fA,
                                                                const uint8_t *__restrict__ fB,
                                                                uint32_t *coef_rw,
                                                                const float *__restrict__ u_in,
                                                                const float *__restrict__ v_in, const StripGeom g,
                                                                const float ilambda,
                                                                unsigned *__restrict__ eps_out, const int eps_stride,
                                                                unsigned long long *__restrict__ stamps,
                                                                const float eps_thr, const PersistArgs pa)
{
    strip_body<R, NTMAX, EPS, E0, DERIV, true>(coef_rw, u_in, v_in, nullptr, nullptr, g, ilambda, eps_out, eps_stride, stamps, eps_thr,
                                               fA, fB, coef_rw, FrameSrc{g.P, g.P, nullptr, nullptr}, pa);
}

// ------------------------------------------------------------------------------------------
// a2, form 4: "folded" strips.  Same register-resident scheme as k_jacobi_strip, but one wavefront
// holds TWO vertically adjacent strips of 128 columns: lanes 0-31 the upper one (rows top->bottom
// in registers 0..R-1), lanes 32-63 the lower one in MIRRORED order (register r = block row
// 2R-1-r).  Both halves then have their wave-internal boundary at register row R-1 and their
// outer edge at register row 0, so
//   * the inner boundary is exchanged inside the wavefront (v_permlane32_swap, no LDS),
//   * each wavefront publishes ONE row per half through LDS (2 ds_write_b128 + 2 ds_read_b128 per
//     sweep instead of 4 + 4) -- the LDS edge-row exchange is what bounds the strip kernel,
//   * no per-half selects are needed: the update is symmetric in up/down, so the lower half simply
//     walks its rows in the opposite direction.
// The DPP wave shifts cross the lane 31/32 seam, which is harmless: lanes 31 and 32 sit on the
// region's right / left edge (junk the validity argument tolerates).
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float lane_xor32(float x, bool lower)
{
    // value of the same register in lane (l ^ 32)
    const unsigned b = __float_as_uint(x);
    const auto r = __builtin_amdgcn_permlane32_swap(b, b, false, false); // r[0] = {lo, lo}, r[1] = {hi, hi}
    return __uint_as_float(lower ? r[0] : r[1]);
}

// E0 = parity of pixel p0 of register row 0 of BOTH halves: yb has the parity of T (CH is even) and the lower half's
// reversed order turns its rows' parities around (strip_body explains the reversal), so one code path serves both.
template <int R, int NTMAX, int EPS, int E0, bool DERIV> // EPS: 0 none, 1 Eps of every sweep, 2 witness, 3 witness + last sweep (strip_body)
__device__ __forceinline__ void fold_body(const uint32_t *__restrict__ coef,
                                                       const float *__restrict__ u_in,
                                                       const float *__restrict__ v_in,
                                                       float *__restrict__ u_out,
                                                       float *__restrict__ v_out, const StripGeom g,
                                                       const float ilambda,
                                                       unsigned *__restrict__ eps_out, const int eps_stride,
                                                       unsigned long long *__restrict__ stamps,
                                                       const float eps_thr, const uint8_t *__restrict__ fA,
                                                       const uint8_t *__restrict__ fB, uint32_t *__restrict__ coef_w)
{
    extern __shared__ __attribute__((aligned(16))) float4 ex[]; // [2 buf][NW][2 half][2 plane][32], then Eps
    unsigned long long st0 = 0, sr0 = 0, st1 = 0, st2 = 0;
    if (stamps) { st0 = __builtin_amdgcn_s_memtime(); sr0 = __builtin_amdgcn_s_memrealtime(); }
    const int lane = threadIdx.x & 63, hl = lane & 31;
    const bool lower = lane >= 32;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int NW = g.NW;
    float *eps_lds = (float *)(ex + (size_t)2 * NW * 2 * 2 * 32);
    const TileId tl = tile_decode<true, true>(g); // (the pair kept scalar: no register of a lane)
    const int rx0 = tl.bx * g.CW - g.HX;
    const int x0 = rx0 + 4 * hl;
    const int yb = tl.by * g.CH - g.T + w * 2 * R; // first block row of this wavefront
    const long long base = (long long)tl.pair * g.plane;
    const bool xin = group_inside(x0, g.W);
    auto blk_row = [&](int r) { return lower ? 2 * R - 1 - r : r; }; // row of the wavefront's block that register row r holds
    auto image_row = [&](int r) { return yb + blk_row(r); };
    const auto lane_id = [&]() { return lane; };

    f2 uP[R], uQ[R], vP[R], vQ[R];
    RowCoef cf[R];
    float4 lu[R], lv[R];
    uint4 lc[R];
    const bool side = !(rx0 >= 0 && rx0 + 128 <= g.W); // workgroup-uniform
    HS_LOAD_PHASE(R, DERIV, side, xin, x0, base, image_row, lu, lv, lc, uP, uQ, vP, vQ, cf);
    // (the wave shifts in strip_derive cross the lane 31/32 seam like those of the sweep: region-edge columns)
    if constexpr (DERIV) {
        strip_derive<R>(fA, fB, g, base, x0, lower ? yb + 2 * R - 1 : yb, lower ? -1 : 1, xin, lc);
#pragma unroll
        for (int r = 0; r < R; r++) unpack(lu[r], lv[r], lc[r], ilambda, uP[r], uQ[r], vP[r], vQ[r], cf[r]);
    }
    // core membership: per lane (the two halves hold different rows); skip distances: per wavefront
    unsigned rowcore = 0;
    int rdist[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int jl = w * 2 * R + blk_row(r), y = image_row(r); // (per lane: the two halves hold different rows)
        if (HS_ROW_IN_CORE(jl, y, g.T, g.CH, g.H)) rowcore |= 1u << r;
        const int du = row_dist(w * 2 * R + r, g.T, g.CH), dd = row_dist(w * 2 * R + 2 * R - 1 - r, g.T, g.CH);
        rdist[r] = du < dd ? du : dd; // the row is computed while either half still needs it
    }
    const bool lanecore = lane_in_core(x0, 4 * hl, g);
    const int pr = g.W - 1 - x0;
    if (DERIV && lanecore) store_deriv_rows<R>(coef_w, g, base, x0, rowcore, image_row, lc);

#define HF_ROW(r, PE, SC, SP)                                                                      \
    do {                                                                                           \
        if (rdist[r] <= last) {                                                                    \
            f2 ouP, ouQ, ovP, ovQ;                                                                 \
            if (EM == 1) { ouP = uP[r]; ouQ = uQ[r]; ovP = vP[r]; ovQ = vQ[r]; }                   \
            strip_row_update<PE>(uP[r], uQ[r], vP[r], vQ[r], SC, SP, cf[r]);                       \
            if (EM == 1) {                                                                         \
                if (((rowcore >> (r)) & 1u) && lanecore) {                                         \
                    /* image columns of the group are p0 .. p(pr); P = (p0, p3), Q = (p1, p2) */   \
                    e = fmaxf(e, fmaxf(fabsf(sweep_diff(ouP.x, uP[r].x)), fabsf(sweep_diff(ovP.x, vP[r].x))));           \
                    if (pr >= 1) e = fmaxf(e, fmaxf(fabsf(sweep_diff(ouQ.x, uQ[r].x)), fabsf(sweep_diff(ovQ.x, vQ[r].x)))); \
                    if (pr >= 2) e = fmaxf(e, fmaxf(fabsf(sweep_diff(ouQ.y, uQ[r].y)), fabsf(sweep_diff(ovQ.y, vQ[r].y)))); \
                    if (pr >= 3) e = fmaxf(e, fmaxf(fabsf(sweep_diff(ouP.y, uP[r].y)), fabsf(sweep_diff(ovP.y, vP[r].y)))); \
                }                                                                                  \
            }                                                                                      \
        }                                                                                          \
        __builtin_amdgcn_sched_barrier(0);                                                         \
    } while (0)
#define HF_CROSS(S, PE, A, B)                                                                      \
    do {                                                                                           \
        if (rdist[A] <= last || rdist[B] <= last)                                                  \
            cross_rows<PE>(S, uP[A], uQ[A], vP[A], vQ[A], uP[B], uQ[B], vP[B], vQ[B]);             \
    } while (0)
    // slot of (buffer, wavefront, half): two planes of 32 float4
#define HF_SLOT(buf, ww, hh) (ex + ((size_t)(((buf) * NW + (ww)) * 2 + (hh)) * 2) * 32)
#define HF_PUBLISH(buf)                                                                            \
    do {                                                                                           \
        float4 *exw = HF_SLOT(buf, w, lower ? 1 : 0) + hl;                                         \
        exw[0] = make_float4(uP[0].x, uP[0].y, uQ[0].x, uQ[0].y);                                  \
        exw[32] = make_float4(vP[0].x, vP[0].y, vQ[0].x, vQ[0].y);                                 \
    } while (0)

    HF_PUBLISH(0);
    __syncthreads();
    if (stamps) st1 = __builtin_amdgcn_s_memtime();
    // outer neighbour: upper half <- bottom row of the wavefront above (its half 1),
    //                  lower half <- top row of the wavefront below (its half 0);
    // at the region edge the wavefront's own slot stands in (junk the validity argument tolerates)
    const int wo = lower ? (w < NW - 1 ? w + 1 : w) : (w > 0 ? w - 1 : w);
    const int ho = lower ? (w < NW - 1 ? 0 : 1) : (w > 0 ? 1 : 0);
    int seen_n = 0; // EPS == 2: sweeps in which some lane of this wavefront saw a change >= eps_thr
    const unsigned long long wit_mask = __builtin_amdgcn_ballot_w64((rowcore & 1u) && lanecore); // lanes whose answer counts
    // one sweep in Eps mode EM (run_sweeps)
    auto sweep = [&](const int s, auto em_tag) __attribute__((always_inline)) {
        constexpr int EM = decltype(em_tag)::value;
        const int last = g.T - 1 - s; // rows with rdist <= last are still swept
        const float thr_s = __int_as_float(__float_as_int(eps_thr) + ((s + 1) << 24)); // eps_thr * 4^(s+1), as in the strip kernel
        const float4 *eo = HF_SLOT(s & 1, wo, ho) + hl;
        const float4 h4u = eo[0], h4v = eo[32];
        const f2 ouP_ = f2{h4u.x, h4u.y}, ouQ_ = f2{h4u.z, h4u.w}, ovP_ = f2{h4v.x, h4v.y}, ovQ_ = f2{h4v.z, h4v.w};
        // inner neighbour: the other half's register row R-1 (old values), in-register exchange
        const f2 iuP = f2{lane_xor32(uP[R - 1].x, lower), lane_xor32(uP[R - 1].y, lower)};
        const f2 iuQ = f2{lane_xor32(uQ[R - 1].x, lower), lane_xor32(uQ[R - 1].y, lower)};
        const f2 ivP = f2{lane_xor32(vP[R - 1].x, lower), lane_xor32(vP[R - 1].y, lower)};
        const f2 ivQ = f2{lane_xor32(vQ[R - 1].x, lower), lane_xor32(vQ[R - 1].y, lower)};
        float e = 0.f;
        // register rows 0 .. R-1, from the published outer edge towards the inner boundary: each row needs the cross
        // sums of the boundary above it (kept from the previous row) and below it (new); row 0 goes to the LDS as soon
        // as it is done, so that the write drains under the other rows
        const float w0 = uP[0].x; // witness: the published row's u at column x0 before the sweep
        Cross sp, sc;
        if (rdist[0] <= last) cross_rows<E0 ^ 1>(sp, ouP_, ouQ_, ovP_, ovQ_, uP[0], uQ[0], vP[0], vQ[0]);
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int rn = r + 1 < R ? r + 1 : r;
            if (r == R - 1) {
                if (rdist[r] <= last) {
                    if (r & 1) cross_rows<E0 ^ 1>(sc, uP[r], uQ[r], vP[r], vQ[r], iuP, iuQ, ivP, ivQ);
                    else cross_rows<E0>(sc, uP[r], uQ[r], vP[r], vQ[r], iuP, iuQ, ivP, ivQ);
                }
            } else if (r & 1) HF_CROSS(sc, E0 ^ 1, r, rn);
            else HF_CROSS(sc, E0, r, rn);
            if (r & 1) HF_ROW(r, E0 ^ 1, sc, sp);
            else HF_ROW(r, E0, sc, sp);
            if (r == 0) {
                // witness (strip_body explains it): old and new value of the published row at column x0
                if (EM == 2)
                    seen_n += (__builtin_amdgcn_ballot_w64(fabsf(sweep_diff(w0, uP[0].x)) >= thr_s) & wit_mask) != 0 ? 1 : 0;
                if (s + 1 < g.T) HF_PUBLISH((s + 1) & 1);
            }
            sp = sc;
        }
        if constexpr (EM == 1) HS_EPS_FOLD_SWEEP(EPS, e, s, w, NW, lane, eps_lds, eps_out, eps_stride); // (e: core pixels only, HF_ROW)
        if (s + 1 < g.T) __syncthreads();
    };
    run_sweeps<EPS, true>(g.T, sweep);
    eps_tail<EPS, false>(g.T, seen_n, false, w, NW, lane_id, eps_lds, eps_out, eps_out, eps_stride); // (every wavefront looks in every sweep)
#undef HF_ROW
#undef HF_CROSS
#undef HF_PUBLISH
#undef HF_SLOT
    if (stamps) st2 = __builtin_amdgcn_s_memtime();

    if (lanecore) store_flow_rows<R>(u_out, v_out, g, base, x0, rowcore, image_row, uP, uQ, vP, vQ);
    if (stamps && threadIdx.x == 0) store_stamps(stamps, st0, sr0, st1, st2, tl.tile);
}

template <int R, int NTMAX, int EPS, int E0>
__global__ __launch_bounds__(NTMAX) void k_jacobi_fold(const uint32_t *__restrict__ coef,
                                                       const float *__restrict__ u_in,
                                                       const float *__restrict__ v_in,
                                                       float *__restrict__ u_out,
                                                       float *__restrict__ v_out, const StripGeom g,
                                                       const float ilambda,
                                                       unsigned *__restrict__ eps_out, const int eps_stride,
                                                       unsigned long long *__restrict__ stamps,
                                                       const float eps_thr)
{
    fold_body<R, NTMAX, EPS, E0, false>(coef, u_in, v_in, u_out, v_out, g, ilambda, eps_out, eps_stride, stamps, eps_thr,
                                    nullptr, nullptr, nullptr);
}

// The folded kernel as the first launch of a solve, derivative pass included (see k_jacobi_strip_deriv).
template <int R, int NTMAX, int EPS, int E0>
__global__ __launch_bounds__(NTMAX) void k_jacobi_fold_deriv(const uint8_t *__restrict__ fA,
                                                             const uint8_t *__restrict__ fB,
                                                             uint32_t *__restrict__ coef_w,
                                                             const float *__restrict__ u_in,
                                                             const float *__restrict__ v_in,
                                                             float *__restrict__ u_out,
                                                             float *__restrict__ v_out, const StripGeom g,
                                                             const float ilambda,
                                                             unsigned *__restrict__ eps_out, const int eps_stride,
                                                             unsigned long long *__restrict__ stamps,
                                                             const float eps_thr)
{
    fold_body<R, NTMAX, EPS, E0, true>(nullptr, u_in, v_in, u_out, v_out, g, ilambda, eps_out, eps_stride, stamps, eps_thr,
                                   fA, fB, coef_w);
}

#undef HS_ROW_IN_CORE
#undef HS_EPS_FOLD_SWEEP
#undef HS_LOAD_PHASE
#undef HS_MIRROR_ROW

} // namespace hsk
