// Batched Hungarian assignment on the device: scipy.optimize.linear_sum_assignment for P independent float64 cost matrices, one
// wavefront per problem, problems side by side across the CUs (the algorithm and why it has to be scipy's, step for step: lsap.hpp).
// Replaces the host solver behind `hungarian=True` of tools/nusc_shasta/pub_tracker.py:103-106 / pub_tracker_merged.py:131-134 and
// behind mot_3d/association.py `mode='bipartite'`; the matrix never leaves the device.
#include "lsap.hpp"

namespace shasta {

constexpr int LSAP_CAP = 1024;  // rows and columns of one problem: solver state of 1024 x 1024 = 34 KB of static LDS

struct LsapArgs {
    const double* cost;  // (P, Nmax, Mmax)
    const int* n;        // (P,)
    const int* m;        // (P,)
    int* col_of_row;     // (P, Nmax)
    int* status;         // (P,)
    int* over;           // (P, Nmax) or nullptr: 1 when the row's pair costs more than over_above
    double clip;         // costs above it count as it (+inf: none); the matrix itself is left alone
    double over_above;
    int Nmax, Mmax;
};

__global__ __launch_bounds__(64) void lsap_kernel(LsapArgs a) {
    __shared__ __attribute__((aligned(8))) unsigned char lds[lsap_state_bytes(LSAP_CAP, LSAP_CAP)];
    const int p = blockIdx.x, lane = threadIdx.x;
    const int n = a.n[p], m = a.m[p];
    const double* C = a.cost + (size_t)p * a.Nmax * a.Mmax;
    int* out = a.col_of_row + (size_t)p * a.Nmax;
    for (int i = lane; i < a.Nmax; i += 64) {
        out[i] = -1;
        if (a.over) a.over[(size_t)p * a.Nmax + i] = 0;
    }
    if (n < 0 || m < 0 || n > a.Nmax || m > a.Mmax) {  // sizes that do not fit the batch's padding: nothing is read
        if (lane == 0) a.status[p] = 1;
        return;
    }
    if (n == 0 || m == 0) {
        if (lane == 0) a.status[p] = 0;
        return;
    }
    // scipy refuses NaN and -inf before it solves; +inf is a forbidden pair and may make the problem infeasible
    bool bad = false;
    for (int i = 0; i < n; ++i)
        for (int j = lane; j < m; j += 64) {
            const double c = C[(size_t)i * a.Mmax + j];
            bad = bad || c != c || c == -INFINITY;
        }
    if (__any(bad)) {
        if (lane == 0) a.status[p] = 1;
        return;
    }
    const LsapState s = lsap_carve(lds, LSAP_CAP, LSAP_CAP);
    const size_t ld = a.Mmax;
    const double clip = a.clip;
    auto cost = [C, ld, clip](int i, int j) {
        const double c = C[(size_t)i * ld + j];
        return c > clip ? clip : c;
    };
    int* over = a.over ? a.over + (size_t)p * a.Nmax : nullptr;
    int st;
    if (n <= m) {
        st = lsap_solve(s, n, m, cost);
        for (int i = lane; st == 0 && i < n; i += 64) {
            const int j = s.col4row[i];
            out[i] = j;
            if (over) over[i] = cost(i, j) > a.over_above ? 1 : 0;
        }
    } else {  // more rows than columns: the transposed problem, pairs swapped back
        st = lsap_solve(s, m, n, [cost](int j, int i) { return cost(i, j); });
        for (int j = lane; st == 0 && j < m; j += 64) {
            const int i = s.col4row[j];
            out[i] = j;
            if (over) over[i] = cost(i, j) > a.over_above ? 1 : 0;
        }
    }
    if (lane == 0) a.status[p] = st;
}

}  // namespace shasta

using namespace shasta;

static int lsap_launch(const double* cost, const int32_t* n, const int32_t* m, int problems, int Nmax, int Mmax, double clip,
                       double over_above, int32_t* col_of_row, int32_t* over, int32_t* status, shasta_stream_t stream) {
    SHASTA_REQUIRE(problems >= 0 && Nmax >= 1 && Mmax >= 1, "lsap: bad size");
    if (Nmax > LSAP_CAP || Mmax > LSAP_CAP) {
        set_error_msg("lsap: at most 1024 rows and 1024 columns per problem (the solver state of one problem lives in LDS)");
        return SHASTA_E_UNSUPPORTED;
    }
    if (problems == 0) return SHASTA_OK;
    SHASTA_REQUIRE(cost && n && m && col_of_row && status, "lsap: null pointer");
    LsapArgs a{cost, n, m, col_of_row, status, over, clip, over_above, Nmax, Mmax};
    hipLaunchKernelGGL(lsap_kernel, dim3(problems), dim3(64), 0, as_stream(stream), a);
    return check_launch("lsap");
}

extern "C" int shasta_lsap_f64(const double* cost, const int32_t* n, const int32_t* m, int problems, int Nmax, int Mmax,
                               int32_t* col_of_row, int32_t* status, shasta_stream_t stream) {
    return lsap_launch(cost, n, m, problems, Nmax, Mmax, INFINITY, INFINITY, col_of_row, nullptr, status, stream);
}

extern "C" int shasta_lsap_clip_f64(const double* cost, const int32_t* n, const int32_t* m, int problems, int Nmax, int Mmax, double clip,
                                    double over_above, int32_t* col_of_row, int32_t* over, int32_t* status, shasta_stream_t stream) {
    SHASTA_REQUIRE(clip == clip && over_above == over_above && (over || problems == 0), "lsap_clip: NaN bound or null pointer");
    return lsap_launch(cost, n, m, problems, Nmax, Mmax, clip, over_above, col_of_row, over, status, stream);
}
