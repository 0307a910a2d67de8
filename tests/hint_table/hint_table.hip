// TEST-ONLY x86 build of the order hint's launch-order table (csrc/dcol_device.hpp
// hint_fill_window_scalar and the position arithmetic under it, csrc/dcol_launch.hpp
// hint_windows), so tests/test_hint_table.py can check the table without a GPU.  Built by
// tests/hint_table/Makefile into tests/hint_table/libhint_table.so.
#include <cstdint>

#include "../../dcol-trajectory-optimization_amd/csrc/dcol_device.hpp"
#include "../../dcol-trajectory-optimization_amd/csrc/dcol_launch.hpp"

using namespace dcol;

extern "C" {

int32_t hint_table_windows(int64_t n, int32_t lpp, int32_t ww) { return hint_windows(n, lpp, ww); }
int32_t hint_table_window_len(int64_t n, int64_t win, int32_t ws) { return hint_window_len(n, win, ws); }
int64_t hint_table_entry_index(int64_t win, int32_t pos, int32_t ppw, int32_t wins) {
    return hint_entry_index(win, pos, ppw, wins);
}
int64_t hint_table_solve_blocks(int32_t wins, int32_t ww) { return hint_solve_blocks(wins, ww); }

// The table of one launch (slots [slot0, slot0 + n) of a plan of B pairs, lpp lanes per pair,
// ww waves per window) from the hint bytes h[B], as the filler waves leave it: every window of
// the padded grid through hint_fill_window_scalar, into tab + tab0.  Returns the windows.
int32_t hint_table_build(int64_t B, int64_t slot0, int64_t n, int32_t lpp, int32_t ww, const uint8_t* h,
                         const int32_t* perm, const int32_t* s1, const int32_t* s2, int32_t* tab, int64_t tab0) {
    KArgs a{};
    a.B = B;
    a.slot0 = slot0;
    a.n = n;
    a.perm = perm;
    a.s1 = s1;
    a.s2 = s2;
    a.hint_r = h;
    a.hint_ww = ww;
    a.hint_wins = hint_windows(n, lpp, ww);
    a.hint_tab_w = reinterpret_cast<HintEntry*>(tab);
    a.hint_tab0 = tab0;
    for (int64_t win = 0; win < a.hint_wins; ++win) hint_fill_window_scalar(a, win, 64 / lpp);
    return a.hint_wins;
}

}  // extern "C"
