// Host check of the rule for the streaming kernels' 16-byte form
// (quadiron_amd/csrc/qi_internal.h: rows_vec and the locate's and the
// fingerprint's use of it), against values written out here.  Stand-alone:
// links nothing of the library and touches no device (run by
// tests/test_rows_vec.py under ASan + UBSan).
#include <cstdio>
#include <cstdlib>

#include "../../quadiron_amd/csrc/qi_internal.h"

using namespace qi;

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

int main()
{
    alignas(16) static unsigned char buf[64];
    const void* al = buf;       // a multiple of 16 bytes
    const void* off = buf + 2;  // one symbol past it

    // the predicate: base and both strides (in u16) multiples of 16 bytes
    CHECK(rows_vec(al, 8, 16));
    CHECK(rows_vec(al, 16, 8));
    CHECK(!rows_vec(off, 8, 16));
    CHECK(!rows_vec(al, 12, 16) && !rows_vec(al, 16, 12));
    CHECK(rows_vec(al, 0, 0) && rows_vec(al, 0, 8) && !rows_vec(off, 0, 0));
    CHECK(rows_vec(al, -8, 16) && rows_vec(al, 16, -4096) && !rows_vec(al, -12, 16));

    // locate: coded always counts, data only below a split
    CHECK(locate_rows_vec(0, off, 12, 12, al, 8, 16));
    CHECK(!locate_rows_vec(4, off, 8, 8, al, 8, 16));
    CHECK(!locate_rows_vec(4, al, 12, 8, al, 8, 16));
    CHECK(locate_rows_vec(4, al, 8, 8, al, 8, 16));
    CHECK(!locate_rows_vec(0, al, 8, 8, off, 8, 16) && !locate_rows_vec(0, al, 8, 8, al, 8, 12));

    // fingerprint: a region that is not held does not count, data only below
    // a split, and the first column is a multiple of 8
    CHECK(fingerprint_rows_vec(0, 4, al, 8, 8, nullptr, 12, 12));
    CHECK(!fingerprint_rows_vec(0, 4, al, 8, 8, al, 12, 8));
    CHECK(fingerprint_rows_vec(0, 4, nullptr, 12, 12, al, 8, 8));
    CHECK(fingerprint_rows_vec(0, 0, off, 12, 12, al, 8, 8));
    CHECK(!fingerprint_rows_vec(0, 4, off, 8, 8, al, 8, 8));
    CHECK(!fingerprint_rows_vec(4, 4, al, 8, 8, al, 8, 8));
    CHECK(fingerprint_rows_vec(8, 4, al, 8, 8, al, 8, 8));

    std::printf("ALL OK\n");
    return 0;
}
