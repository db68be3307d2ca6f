// Host-only driver for tests/test_matrix_route.py: matrix_route
// (quadiron_amd/csrc/matrix_route.h, compiled by plain g++) over the inputs
// read from stdin, one per line:
//   R kin words buf align in_marks out_marks ids route two
// (KP = matrix_kp(kin)); prints per line "<err>|<to_string of the route>".
#include <cstdio>

#include "../../quadiron_amd/csrc/matrix_route.h"

int main()
{
    int R, kin, buf, align, in, out, ids, route, two;
    long long words;
    while (std::scanf("%d %d %lld %d %d %d %d %d %d %d", &R, &kin, &words, &buf, &align, &in, &out,
                      &ids, &route, &two) == 10) {
        const qi::MatRouteIn q{qi::MatLayout{R, kin, qi::matrix_kp(kin)}, words, buf != 0, align,
                               in != 0, out != 0, ids != 0, route != 0, two != 0};
        const qi::MatRoute r = qi::matrix_route(q);
        std::printf("%d|%s\n", r.err, qi::to_string(r).c_str());
    }
    return 0;
}
