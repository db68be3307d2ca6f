// Host-only driver for tests/test_matrix_route.py: row_extent
// (quadiron_amd/csrc/matrix_route.h, compiled by plain g++) over the inputs
// read from stdin, one per line:
//   rows rs words
// prints the extent per line.
#include <cstdio>

#include "../../quadiron_amd/csrc/matrix_route.h"

int main()
{
    long long rows, rs, words;
    while (std::scanf("%lld %lld %lld", &rows, &rs, &words) == 3)
        std::printf("%u\n", qi::row_extent(rows, rs, words));
    return 0;
}
