// TEST-ONLY x86 build of the order-hint permutation rule (csrc/dcol_device.hpp:
// dcol::hint_position, the scalar form of the solve kernel's prologue), for
// tests/test_order_hint.py (tests/emul_hint/libdcol_hint_emul.so).
#include <cstdint>

#include "../../dcol-trajectory-optimization_amd/csrc/dcol_device.hpp"

// order[p] = the slot of a window of len hint bytes h that takes position p; entries the
// rule does not reach keep the caller's prefill
extern "C" void dcol_emul_hint_order(const uint8_t* h, int32_t len, int32_t* order) {
    for (int32_t i = 0; i < len; ++i) {
        const int p = dcol::hint_position(h, len, i);
        if (p >= 0 && p < len) order[p] = i;
    }
}
