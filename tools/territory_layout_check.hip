// territory_layout_check.hip -- host-only check of qs_terr_layout (csrc/territory_layout.h), for a sanitizer build:
//   make -C <package>/csrc layout-check
// builds it with -fsanitize=address,undefined on the host side and runs it; no GPU and no HIP call is involved.
// For a range of grid sizes, centroid and bot counts and both optional arrays on and off it carves the workspace over a
// heap block of exactly the bytes the sizing pass reports, writes every piece over its full extent (an overrun of the
// block is the sanitizer's to find), and checks alignment, order, that no two pieces overlap, and that a piece that was
// not asked for is a null pointer that takes no bytes.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "territory_layout.h"

struct Piece { const char *name; char *p; size_t bytes; };

static int check(int size, size_t n_cent, size_t n_bots, bool want_owner, bool want_cost)
{
    const QsTerrLayout Q = qs_terr_layout(nullptr, size, n_cent, n_bots, want_owner, want_cost);
    if (Q.key || Q.slot || Q.owner || Q.cost || Q.tg.pair_bot) { fprintf(stderr, "sizing pass handed out a pointer\n"); return 1; }
    char *ws = (char *)aligned_alloc(256, Q.bytes ? Q.bytes : 256);
    if (!ws) { fprintf(stderr, "no memory for %zu bytes\n", Q.bytes); return 1; }
    const QsTerrLayout L = qs_terr_layout(ws, size, n_cent, n_bots, want_owner, want_cost);
    const size_t cells = (size_t)size * size, n_end = n_cent + n_bots;
    const QsTgtLayout &S = L.tg;
    const Piece pc[] = {
        {"key", (char *)L.key, L.field_cells * 8}, {"slot", (char *)L.slot, n_bots * 8}, {"area", (char *)L.area, n_bots * 8},
        {"box", (char *)L.box, n_bots * 16}, {"count", (char *)S.count, 32}, {"xy", (char *)S.xy, n_end * 16},
        {"cell", (char *)S.cell, n_end * 8}, {"coff", (char *)S.coff, n_cent * 4}, {"tgt_idx", (char *)S.tgt_idx, n_bots * 8},
        {"tgt_cost", (char *)S.tgt_cost, n_bots * 4}, {"tgt_status", (char *)S.tgt_status, n_bots * 4},
        {"pair", (char *)S.pair, n_bots * 16}, {"pair_bot", (char *)S.pair_bot, n_bots * 4},
        {"cent_owner", (char *)L.cent_owner, n_cent * 4}, {"cent_cost", (char *)L.cent_cost, n_cent * 4},
        {"tgt_xy", (char *)L.tgt_xy, n_bots * 16}, {"owner", (char *)L.owner, want_owner ? cells * 2 : 0},
        {"cost", (char *)L.cost, want_cost ? cells * 4 : 0}};
    int bad = 0;
    if (L.bytes != Q.bytes) { fprintf(stderr, "bytes differ between the passes: %zu, %zu\n", Q.bytes, L.bytes); bad = 1; }
    if ((L.owner != nullptr) != want_owner || (L.cost != nullptr) != want_cost) { fprintf(stderr, "optional piece: wrong presence\n"); bad = 1; }
    if (L.field_cells < cells || L.field_cells % (PL_T * PL_T)) { fprintf(stderr, "field_cells %zu for size %d\n", L.field_cells, size); bad = 1; }
    char *end = ws;
    for (size_t i = 0; i < sizeof pc / sizeof pc[0]; i++) {
        if (!pc[i].p) continue;
        if (((size_t)(pc[i].p - ws) & 255) || pc[i].p < end || pc[i].p + pc[i].bytes > ws + L.bytes) {
            fprintf(stderr, "%s: offset %zd, %zu bytes, previous end %zd, block %zu\n", pc[i].name, pc[i].p - ws, pc[i].bytes,
                    end - ws, L.bytes);
            bad = 1;
            continue;
        }
        memset(pc[i].p, (int)(i + 1), pc[i].bytes);
        end = pc[i].p + pc[i].bytes;
    }
    for (size_t i = 0; i < sizeof pc / sizeof pc[0] && !bad; i++)          // nothing a later piece wrote reaches an earlier one
        for (size_t k = 0; k < pc[i].bytes; k += pc[i].bytes > 4096 ? pc[i].bytes / 64 : 1)
            if (pc[i].p && (unsigned char)pc[i].p[k] != i + 1) { fprintf(stderr, "%s: overwritten at %zu\n", pc[i].name, k); bad = 1; break; }
    free(ws);
    return bad;
}

int main()
{
    const int sizes[] = {1, 63, 64, 65, 200, 256, 1000};
    const size_t cents[] = {0, 1, 63, 64, 65, 1000}, bots[] = {0, 1, 2, 64, 1023, 1024};
    int bad = 0, n = 0;
    for (int size : sizes)
        for (size_t nc : cents)
            for (size_t nb : bots)
                for (int opt = 0; opt < 4; opt++, n++) bad |= check(size, nc, nb, opt & 1, opt & 2);
    printf("territory layout: %d layouts checked, %s\n", n, bad ? "FAILED" : "ok");
    return bad;
}
