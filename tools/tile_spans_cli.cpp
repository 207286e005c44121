// Stand-alone front of srt_tile_spans.h (plain C++, no HIP): tests/test_tile_spans.py drives it, and the same file is what a sanitizer
// build runs (g++ -fsanitize=address,undefined -I simple_raytracer_amd/csrc tools/tile_spans_cli.cpp).
//
// stdin, any number of cases:   n_objects width height i0 j0 focal   then per object   minx miny minz maxx maxy maxz
//                               (floats as strtof reads them: hexadecimal floats, inf, nan)
// stdout, per case:             on row0 n_rows   then, when on, one line of "x0:n" for every tile row of the frame
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "srt_tile_spans.h"

static bool read_float(float* out) {
    char tok[64];
    if (std::scanf("%63s", tok) != 1) return false;
    char* end = nullptr;
    *out = std::strtof(tok, &end);
    return end != tok && *end == '\0';
}

int main() {
    for (;;) {
        unsigned n = 0, w = 0, h = 0; int i0 = 0, j0 = 0;
        const int got = std::scanf("%u %u %u %d %d", &n, &w, &h, &i0, &j0);
        if (got == EOF) return 0;
        float focal;
        if (got != 5 || n > (1u << 20) || !read_float(&focal)) { std::fprintf(stderr, "malformed case\n"); return 2; }
        std::vector<float> mn(3 * (size_t)n + 1), mx(3 * (size_t)n + 1);
        for (unsigned k = 0; k < n; k++) {
            for (int a = 0; a < 3; a++) if (!read_float(&mn[3 * k + a])) { std::fprintf(stderr, "malformed box\n"); return 2; }
            for (int a = 0; a < 3; a++) if (!read_float(&mx[3 * k + a])) { std::fprintf(stderr, "malformed box\n"); return 2; }
        }
        TileSpans ts;
        const bool on = tile_spans(mn.data(), mx.data(), n, w, h, i0, j0, focal, &ts);
        std::printf("%d %u %u\n", on ? 1 : 0, on ? (unsigned)ts.row0 : 0u, on ? (unsigned)ts.n_rows : 0u);
        if (on) {
            const unsigned gy = (h + 7u) / 8u;
            for (unsigned r = 0; r < gy; r++) {      // (the table's rows count from row0)
                const bool in = r >= ts.row0 && r < (unsigned)ts.row0 + ts.n_rows;
                std::printf("%u:%u%c", in ? (unsigned)ts.row[r - ts.row0].x0 : 0u, in ? (unsigned)ts.row[r - ts.row0].n : 0u, r + 1 == gy ? '\n' : ' ');
            }
        }
    }
}
