// linalg_runner.cpp — test-only driver of csrc/host_linalg.hpp as the host compiler sees it (g++, no HIP: RSREG_HD is
// empty).  Built and run by tests/umeyama_cases.py.
//
//   linalg_runner <cases> <results>
//
// <cases>: records, each an int32 op, an int32 count and the op's f64 payload; <results>: the answers in the same order, raw.
//   op 1  cold solve        count x sums[17]                  -> count x (int32 ok, T f32[16])
//   op 2  warm sequence     V0[9], count x sums[17]           -> count x (int32 ok, T f32[16], V f64[9]); V is carried
//   op 3  the two SVDs      count x A[9]                      -> count x (jacobi_svd3 U[9] s[3] V[9], jacobi_svd<3> U[9] s[3] V[9])
//   op 4  eig_sym3          count x A[9]                      -> count x (evals[3], evecs[9])
//   op 5  svd_solve<6>      count x (A[36], b[6])             -> count x x[6]
//   op 6  the 6 x 6 SVD     count x A[36]                     -> count x s[6]
//   op 7  jacobi_svd3 warm  count x (V0[9], A[9])             -> count x (U[9] s[3] V[9])
#include <cstdint>
#include <cstdio>
#include <vector>

#include "host_linalg.hpp"

using namespace rsreg;

namespace {

bool get(FILE *f, void *p, size_t bytes) { return std::fread(p, 1, bytes, f) == bytes; }
bool put(FILE *f, const void *p, size_t bytes) { return std::fwrite(p, 1, bytes, f) == bytes; }

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) {
        std::fprintf(stderr, "usage: linalg_runner <cases> <results>\n");
        return 2;
    }
    FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) {
        std::fprintf(stderr, "cannot open %s or %s\n", argv[1], argv[2]);
        return 2;
    }
    int32_t head[2];
    long records = 0;
    while (get(in, head, sizeof(head))) {
        const int op = head[0], count = head[1];
        if (count < 0 || count > (1 << 20)) return 3;
        bool ok = true;
        if (op == 1 || op == 2) {
            double v[9];
            if (op == 2 && !get(in, v, sizeof(v))) return 3;
            for (int c = 0; c < count && ok; ++c) {
                double sums[17];
                if (!get(in, sums, sizeof(sums))) return 3;
                Mat4f t = Mat4f::identity();
                const int32_t solved = (op == 1 ? umeyama_from_sums(sums, t) : umeyama_from_sums(sums, t, v)) ? 1 : 0;
                ok = put(out, &solved, 4) && put(out, t.m, sizeof(t.m)) && (op == 1 || put(out, v, sizeof(v)));
            }
        } else if (op == 3) {
            for (int c = 0; c < count && ok; ++c) {
                double a[9];
                if (!get(in, a, sizeof(a))) return 3;
                SvdResult<3> r3, rg;
                jacobi_svd3(a, r3);
                jacobi_svd<3>(a, rg);
                ok = put(out, r3.U, 72) && put(out, r3.s, 24) && put(out, r3.V, 72) && put(out, rg.U, 72) && put(out, rg.s, 24) && put(out, rg.V, 72);
            }
        } else if (op == 4) {
            for (int c = 0; c < count && ok; ++c) {
                double a[9], w[3], v[9];
                if (!get(in, a, sizeof(a))) return 3;
                eig_sym3(a, w, v);
                ok = put(out, w, sizeof(w)) && put(out, v, sizeof(v));
            }
        } else if (op == 5) {
            for (int c = 0; c < count && ok; ++c) {
                double a[36], b[6], x[6];
                if (!get(in, a, sizeof(a)) || !get(in, b, sizeof(b))) return 3;
                svd_solve<6>(a, b, x);
                ok = put(out, x, sizeof(x));
            }
        } else if (op == 6) {
            for (int c = 0; c < count && ok; ++c) {
                double a[36];
                if (!get(in, a, sizeof(a))) return 3;
                SvdResult<6> r;
                jacobi_svd<6>(a, r);
                ok = put(out, r.s, sizeof(r.s));
            }
        } else if (op == 7) {
            for (int c = 0; c < count && ok; ++c) {
                double v0[9], a[9];
                if (!get(in, v0, sizeof(v0)) || !get(in, a, sizeof(a))) return 3;
                SvdResult<3> r;
                jacobi_svd3(a, r, v0);
                ok = put(out, r.U, 72) && put(out, r.s, 24) && put(out, r.V, 72);
            }
        } else {
            std::fprintf(stderr, "unknown op %d\n", op);
            return 3;
        }
        if (!ok) return 4;
        ++records;
    }
    if (std::fclose(out) != 0) return 4;
    std::fclose(in);
    std::printf("linalg_runner: %ld records\n", records);
    return 0;
}
