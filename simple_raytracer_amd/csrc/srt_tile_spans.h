// Which 8x8 tiles of a frame can hold a ray that passes any object's root box: per tile row one span of tiles, from the root boxes'
// projection alone ("Tile spans").  Plain C++, nothing of HIP: the host computes the table per frame, the kernels that take
// it (srt_kernels.h) read it as a by-value argument, and a stand-alone program can compile this file on its own.
//
// Rays are lines through the origin with direction (i, j, focal), i = i0 + column, j = j0 + row (whole pixels: no sub-pixel offset); the reference's slab
// test (intersectRayAabbNoOrigin) has no t >= 0 clause, so a box behind the image plane is met as well as one in front.
#pragma once
#include <cmath>
#include <cstdint>

constexpr uint32_t TILE_SPAN_ROWS = 512;      // room for this many tile rows (4096 image rows); a taller frame gets no culling
constexpr uint32_t TILE_SPAN_MAX_OBJECTS = 4096;      // the table is made per render call, in time n_objects x tile rows: a scene of more objects gets no culling

struct alignas(4) TileSpan { uint16_t x0, n; };      // first tile and tile count of a row's span (one 32-bit word: one scalar load)
struct TileSpans {
    uint32_t on;                    // 0: no culling -- the host launches the full grid and the kernels that take no table
    uint16_t row0, n_rows;          // the tile rows any span touches: row0 .. row0 + n_rows - 1
    uint32_t epoch;                 // the records' box epoch the table was made at (set by the host; a captured launch compares it with the device's word)
    TileSpan row[TILE_SPAN_ROWS];   // row[k]: tile row row0 + k -- the trace launch's blockIdx.y is the index, no load waits for another
};
static_assert(sizeof(TileSpans) == 12 + 4 * TILE_SPAN_ROWS, "TileSpans has no implicit padding");

// the widest span: the x extent of the stage-1 grid
inline uint32_t tile_spans_max_n(const TileSpans& ts) {
    uint32_t m = 0;
    for (uint32_t k = 0; k < ts.n_rows; k++) if (ts.row[k].n > m) m = ts.row[k].n;
    return m;
}

// The same table with its rows counted from tile row 0 (row0 = 0, empty spans in front): what a launch over the frame's WHOLE grid
// indexes with blockIdx.y (a launch captured into a graph, srt_kernels.h trace_nq_body)
inline TileSpans tile_spans_from_row_zero(const TileSpans& t) {
    TileSpans o = t;
    o.row0 = 0; o.n_rows = (uint16_t)(t.row0 + t.n_rows);
    for (uint32_t k = 0; k < TILE_SPAN_ROWS; k++) {
        const bool in = k >= t.row0 && k < (uint32_t)t.row0 + t.n_rows;
        o.row[k].x0 = in ? t.row[k - t.row0].x0 : (uint16_t)0; o.row[k].n = in ? t.row[k - t.row0].n : (uint16_t)0;
    }
    return o;
}

// Slices a box part's z range is cut into (tile_spans): 32 for scenes of up to 128 objects, fewer beyond so that a frame never costs more than
// 2 x 4096 rectangles, one at TILE_SPAN_MAX_OBJECTS -- the table is made on every render call
inline uint32_t tile_span_slices(uint32_t n_objects) {
    const uint32_t s = n_objects ? TILE_SPAN_MAX_OBJECTS / n_objects : 32u;
    return s > 32u ? 32u : (s < 1u ? 1u : s);
}

namespace tile_spans_detail {
// a / z over a in [a0, a1] and z in [z0, z1], 0 <= z0 <= z1, z1 > 0 (z = 0 itself excluded: an open end where the part reaches it)
inline void quotient_range(double a0, double a1, double z0, double z1, double* lo, double* hi) {
    *lo = a0 >= 0.0 ? a0 / z1 : (z0 > 0.0 ? a0 / z0 : -INFINITY);
    *hi = a1 <= 0.0 ? a1 / z1 : (z0 > 0.0 ? a1 / z0 : INFINITY);
}
// pixel range [lo, hi] (may be infinite) -> tiles, grown by one pixel on both sides and clamped to 0 .. n_tiles - 1; false: off the frame
// (max(floor(a), 0) <= min(floor(b), n - 1), without a call of floor: 32 slices per box part come through here on every render call)
inline bool tile_range(double lo, double hi, uint32_t n_tiles, uint32_t* t0, uint32_t* t1) {
    const double a = (lo - 1.0) / 8.0, b = (hi + 1.0) / 8.0, n = (double)n_tiles;
    if (!(b >= 0.0) || !(a < n)) return false;      // floor(b) < 0 or floor(a) > n - 1
    *t0 = a > 0.0 ? (uint32_t)a : 0u; *t1 = b < n ? (uint32_t)b : n_tiles - 1u;      // (in range, not negative: the conversion is the floor)
    return *t0 <= *t1;
}
// far bound of slice sl of S over [za, zb]: zb exactly for the last, monotone in sl, never beyond zb
inline double z1_of(double za, double zb, uint32_t sl, uint32_t S) {
    return sl + 1u == S ? zb : std::fmin(za + (zb - za) * (double)(sl + 1u) / (double)S, zb);
}
struct Hull {
    uint32_t x0[TILE_SPAN_ROWS], x1[TILE_SPAN_ROWS]; bool any[TILE_SPAN_ROWS];
    void add(uint32_t tx0, uint32_t tx1, uint32_t ty0, uint32_t ty1) {
        for (uint32_t r = ty0; r <= ty1; r++) {
            if (!any[r]) { any[r] = true; x0[r] = tx0; x1[r] = tx1; }
            else { if (tx0 < x0[r]) x0[r] = tx0; if (tx1 > x1[r]) x1[r] = tx1; }
        }
    }
};
}      // namespace tile_spans_detail

// The frame's table from the objects' root boxes, mn / mx = n_objects x 3 floats.  Returns out->on: false = no culling (a frame or a box the
// rule does not cover), and then nothing else of *out means anything.
//
// Per object, in double precision: the box, every bound moved outwards by 2^-22 of itself and 2^-100 (more than the reference's
// correctly rounded quotients, gradual underflow included, can move the point t * d of a passing ray), is cut at z = 0 into its z > 0 part
// and the mirror image of its z < 0 part ((x, y, z) -> (-x, -y, -z), on the same line); of each part the range of focal * x / z and of
// focal * y / z, by interval arithmetic, is the range of (i, j) whose line meets it.  One rectangle per part cannot follow a trapezoid (a
// ground slab narrows towards the horizon), so the part's z range is cut into tile_span_slices() equal slices, closed and sharing their
// bounds, and each slice gets its own rectangle from its own [z0, z1] and the part's x and y ranges: the point t * d of a passing ray lies
// in one of the slices, and there the argument is the part's.  Each rectangle, grown by one pixel on every side, floored to tiles and
// clamped to the frame, is kept; a row's span is the hull of the rectangles that touch it.
// The pixel of margin: a ray's (i, j) are whole pixels, exact in double, and the rectangle's bounds are evaluated in double with a few
// roundings each -- off by parts in 2^52 of a pixel coordinate, which on a frame is below 2^20.  (The margin used to be a whole tile, kept
// for the half pixel a supersampled frame moves its rays by; such a frame gets no table at all: srt_hip.hip plan_frame.)
// Two exceptions, both kept whole.  A box whose inflated form holds the origin meets every line.  And a bound of exactly 0 on x (y) makes
// the quotient 0 / 0 = NaN in the column i = 0 (row j = 0), whose comparisons reject nothing: that tile column (row) is kept over the
// whole frame.  No other ray sees a NaN: focal is finite and positive, the bounds are finite.
inline bool tile_spans(const float* mn, const float* mx, uint32_t n_objects, uint32_t width, uint32_t height, int32_t i0, int32_t j0,
                       float focal, TileSpans* out) {
    using namespace tile_spans_detail;
    out->on = 0u; out->row0 = 0; out->n_rows = 0; out->epoch = 0u;
    const uint32_t gx = (width + 7u) / 8u, gy = (height + 7u) / 8u;
    if (!width || !height || gy > TILE_SPAN_ROWS || gx > 65535u || n_objects > TILE_SPAN_MAX_OBJECTS) return false;
    if (!(focal > 0.0f) || !std::isfinite(focal)) return false;
    const double LIMIT = std::ldexp(1.0, 100), REL = std::ldexp(1.0, -22), ABS = std::ldexp(1.0, -100);
    for (uint32_t k = 0; k < 3u * n_objects; k++) {
        if (!std::isfinite(mn[k]) || !std::isfinite(mx[k]) || mn[k] > mx[k]) return false;      // (an empty leaf's FLT_MAX box is inverted)
        if (std::fabs((double)mn[k]) > LIMIT || std::fabs((double)mx[k]) > LIMIT) return false;
    }
    Hull h;
    for (uint32_t r = 0; r < gy; r++) h.any[r] = false;
    const double f = (double)focal, ox = (double)i0, oy = (double)j0;      // pixel = focal * x / z - o
    const uint32_t n_slices = tile_span_slices(n_objects);
    for (uint32_t k = 0; k < n_objects; k++) {
        double lo[3], hi[3];
        for (int a = 0; a < 3; a++) {
            const double l = (double)mn[3 * k + a], u = (double)mx[3 * k + a];
            lo[a] = l - (std::fabs(l) * REL + ABS); hi[a] = u + (std::fabs(u) * REL + ABS);
        }
        // the NaN column and row: an exact zero bound, the integer pixel whose i (j) is exactly 0 on the frame
        if ((mn[3 * k] == 0.0f || mx[3 * k] == 0.0f) && i0 <= 0 && (int64_t)-i0 < (int64_t)width) { const uint32_t t = (uint32_t)(-i0) / 8u; h.add(t, t, 0, gy - 1u); }
        if ((mn[3 * k + 1] == 0.0f || mx[3 * k + 1] == 0.0f) && j0 <= 0 && (int64_t)-j0 < (int64_t)height) { const uint32_t t = (uint32_t)(-j0) / 8u; h.add(0, gx - 1u, t, t); }
        if (lo[0] <= 0.0 && hi[0] >= 0.0 && lo[1] <= 0.0 && hi[1] >= 0.0 && lo[2] <= 0.0 && hi[2] >= 0.0) { h.add(0, gx - 1u, 0, gy - 1u); continue; }
        for (int part = 0; part < 2; part++) {
            // part 0: z > 0 as it is; part 1: z < 0 mirrored through the origin
            const double x0 = part ? -hi[0] : lo[0], x1 = part ? -lo[0] : hi[0], y0 = part ? -hi[1] : lo[1], y1 = part ? -lo[1] : hi[1];
            const double zb = part ? -lo[2] : hi[2], za = std::fmax(part ? -hi[2] : lo[2], 0.0);
            if (!(zb > 0.0)) continue;
            // the part's one rectangle first: off the frame, and so is every slice's; and where the part straddles both axes all four edges
            // are set by a slice's NEAR bound, every slice's rectangle lies inside the first one's, and that one is the part's
            double ulo, uhi, vlo, vhi;
            uint32_t tx0, tx1, ty0, ty1;
            quotient_range(y0, y1, za, zb, &vlo, &vhi); quotient_range(x0, x1, za, zb, &ulo, &uhi);
            if (!tile_range(f * vlo - oy, f * vhi - oy, gy, &ty0, &ty1) || !tile_range(f * ulo - ox, f * uhi - ox, gx, &tx0, &tx1)) continue;
            const uint32_t S = zb > za && !(x0 < 0.0 && x1 > 0.0 && y0 < 0.0 && y1 > 0.0) ? n_slices : 1u;
            if (S == 1u) { h.add(tx0, tx1, ty0, ty1); continue; }
            // slice sl is [z(sl), z(sl + 1)], z(0) = za, z(S) = zb exactly, z monotone in sl: neighbours share their bound, nothing of the part is left out
            uint32_t px0 = 1, px1 = 0, py0 = 1, py1 = 0;      // the rectangle added last (none yet): a slice's rectangle inside it adds nothing to the hull
            double z0 = za, z1 = za;
            for (uint32_t sl = 0; sl < S; sl++, z0 = z1) {
                z1 = z1_of(za, zb, sl, S);
                if (!(z1 > 0.0)) continue;      // (only by underflow; the one point of a line through the origin at z = 0 is the origin, the exception's above)
                quotient_range(y0, y1, z0, z1, &vlo, &vhi);
                if (!tile_range(f * vlo - oy, f * vhi - oy, gy, &ty0, &ty1)) continue;      // (a slab's near slices lie below the frame)
                quotient_range(x0, x1, z0, z1, &ulo, &uhi);
                if (tile_range(f * ulo - ox, f * uhi - ox, gx, &tx0, &tx1) && !(tx0 >= px0 && tx1 <= px1 && ty0 >= py0 && ty1 <= py1)) {
                    h.add(tx0, tx1, ty0, ty1);
                    px0 = tx0; px1 = tx1; py0 = ty0; py1 = ty1;
                }
            }
        }
    }
    uint32_t first = gy, last = 0;
    for (uint32_t r = 0; r < gy; r++) if (h.any[r]) { if (r < first) first = r; last = r; }
    // nothing in view: one tile stays (row 0, tile 0), so that the stage-1 launch, its events and counters are what they always are
    if (first == gy) { first = last = 0; h.any[0] = true; h.x0[0] = h.x1[0] = 0; }
    for (uint32_t k = 0; k < TILE_SPAN_ROWS; k++) {
        const bool in = first + k <= last && h.any[first + k];
        out->row[k].x0 = in ? (uint16_t)h.x0[first + k] : (uint16_t)0;
        out->row[k].n = in ? (uint16_t)(h.x1[first + k] - h.x0[first + k] + 1u) : (uint16_t)0;
    }
    out->row0 = (uint16_t)first; out->n_rows = (uint16_t)(last - first + 1u);
    out->on = 1u;
    return true;
}
