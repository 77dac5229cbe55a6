// Stand-alone check of rsp_pcplan.h (tests/test_pcplan_cpu.py): the long-row workgroup count of
// a pulse-compression launch at 1, 2 and 4 rows per workgroup slot.  Prints "ok" or the failures.
#include <cstdio>

#include "rsp_pcplan.h"

static int g_bad = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            ++g_bad;                                                 \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);     \
        }                                                            \
    } while (0)

int main() {
    const int units[7] = {0, 1, 2, 3, 4, 5, 2048};
    // by hand: ceil(u / rows) at one row slot per workgroup (the 1024/4096 pair's long rows)
    const int want[3][7] = {
        {0, 1, 2, 3, 4, 5, 2048},   // rows 1
        {0, 1, 1, 2, 2, 3, 1024},   // rows 2
        {0, 1, 1, 1, 1, 2, 512},    // rows 4
    };
    const int rows[3] = {1, 2, 4};
    for (int r = 0; r < 3; ++r) {
        for (int i = 0; i < 7; ++i) {
            const int n = rsp::pc_blocks(units[i], 1, rows[r]);
            CHECK(n == want[r][i]);
            // every unit has a slot, and the last workgroup holds at least one valid unit
            for (int rpb = 1; rpb <= 4; rpb *= 2) {
                const long long per = (long long)rpb * rows[r];
                const int nb = rsp::pc_blocks(units[i], rpb, rows[r]);
                CHECK(nb * per >= units[i]);
                CHECK(units[i] == 0 ? nb == 0 : (nb - 1) * per < units[i]);
            }
        }
    }
    CHECK(rsp::pc_blocks(-3, 1, 2) == 0 && rsp::pc_blocks(5, 0, 2) == 0 && rsp::pc_blocks(5, 1, 0) == 0);
    CHECK(rsp::pc_blocks((1LL << 31) - 1, 1, 4) == (1 << 29));   // no 32-bit overflow in units + per - 1
    CHECK(rsp::pc_rows_valid(1) && rsp::pc_rows_valid(2) && rsp::pc_rows_valid(4));
    CHECK(!rsp::pc_rows_valid(0) && !rsp::pc_rows_valid(3) && !rsp::pc_rows_valid(8) && !rsp::pc_rows_valid(-1));
    CHECK(rsp::pc_rows_valid(rsp::kPcRowsDefault));
    if (g_bad == 0) std::puts("ok");
    return g_bad ? 1 : 0;
}
