// Host-only driver for tests/test_verify_host.py: matrix_route
// (quadiron_amd/csrc/matrix_route.h, compiled by plain g++, with
// -fsanitize=address,undefined) over the inputs read from stdin, one per
// line, with the verify form as the last field:
//   R kin words buf align in_marks out_marks ids route two verify
// (KP = matrix_kp(kin)); prints per line "<err>|<to_string of the route>".
// With verify = 0 the input is built without naming the field, as the callers
// that predate it do, so the pinned routes are compared through the default.
#include <cstdio>

#include "../../quadiron_amd/csrc/matrix_route.h"

int main()
{
    int R, kin, buf, align, in, out, ids, route, two, verify;
    long long words;
    while (std::scanf("%d %d %lld %d %d %d %d %d %d %d %d", &R, &kin, &words, &buf, &align, &in,
                      &out, &ids, &route, &two, &verify) == 11) {
        qi::MatRouteIn q{qi::MatLayout{R, kin, qi::matrix_kp(kin)}, words, buf != 0, align,
                         in != 0, out != 0, ids != 0, route != 0, two != 0};
        if (verify)
            q.verify = true;
        const qi::MatRoute r = qi::matrix_route(q);
        // a verify route never reports the _both forms, and the other way
        if (r.verify != (verify != 0) || (r.verify && r.both))
            return 2;
        std::printf("%d|%s\n", r.err, qi::to_string(r).c_str());
    }
    return 0;
}
