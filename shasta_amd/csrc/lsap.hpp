// Rectangular linear sum assignment by shortest augmenting paths (Crouse 2016), restated step for step from scipy's
// `rectangular_lsap` so that the returned optimum - not just its cost - is scipy's: the tracker's matrices carry 1e18 for invalid
// pairs, a float64 ulp is 128 there, and which of the equal-cost optima comes out depends on the exact order of the additions and on
// the tie rule of the column scan.  One wavefront solves one problem: the rows are augmented one after the other (serial by nature),
// the scan over the still-open columns of every Dijkstra step runs over the lanes.
//   r       = ((minVal + cost[i][j]) - u[i]) - v[j]      in this order (build flag -ffp-contract=off, no reassociation)
//   index   = where scipy's serial scan `if (spc[j] < lowest || (spc[j] == lowest && row4col[j] == -1))` stops: among the positions
//             of remaining[] holding the minimum, the LAST one with an unassigned column, else the FIRST position
//   remaining[] is kept literally (initialised nc-1 .. 0, closed columns replaced by the last open one): positions decide ties.
#pragma once
#include "common.hpp"

namespace shasta {

// index arrays are 16-bit: capacities stay below 32768 and the state of a 512 x 768 problem fits next to the scene tracker's LDS
struct LsapState {
    double* u;         // [rows]
    double* v;         // [cols]
    double* spc;       // [cols] shortest path costs
    short* col4row;    // [rows] result: column of every row
    short* row4col;    // [cols]
    short* path;       // [cols]
    short* remaining;  // [cols]
    unsigned char* SR; // [rows]
    unsigned char* SC; // [cols]
};

constexpr size_t lsap_state_bytes(int rows, int cols) { return (size_t)8 * (rows + 2 * cols) + (size_t)2 * (rows + 3 * cols) + rows + cols; }

// carve the state out of an 8-byte aligned block of lsap_state_bytes(rows, cols) (rows, cols even)
__device__ __forceinline__ LsapState lsap_carve(void* base, int rows, int cols) {
    LsapState s;
    s.u = reinterpret_cast<double*>(base);
    s.v = s.u + rows;
    s.spc = s.v + cols;
    s.col4row = reinterpret_cast<short*>(s.spc + cols);
    s.row4col = s.col4row + rows;
    s.path = s.row4col + cols;
    s.remaining = s.path + cols;
    s.SR = reinterpret_cast<unsigned char*>(s.remaining + cols);
    s.SC = s.SR + rows;
    return s;
}

struct LsapCand {
    double val;
    int pos;
    bool open;  // column unassigned
};

// total order that a scan in ascending position ends on: smaller value; at equal value an unassigned column beats an assigned one,
// the later of two unassigned ones wins, the earlier of two assigned ones wins
__device__ __forceinline__ bool lsap_better(const LsapCand& a, const LsapCand& b) {
    if (a.val != b.val) return a.val < b.val;
    if (a.open != b.open) return a.open;
    return a.open ? a.pos > b.pos : a.pos < b.pos;
}

// nr <= nc, called by all 64 lanes of the one wavefront of the workgroup; cost(i, j) for 0 <= i < nr, 0 <= j < nc must be free of NaN
// and -inf.  Returns 0 (s.col4row[0 .. nr) holds the assignment) or 2 (infeasible: some row has no finite augmenting path).
template <class Cost>
__device__ int lsap_solve(const LsapState& s, int nr, int nc, Cost cost) {
    const int lane = threadIdx.x;
    for (int i = lane; i < nr; i += 64) {
        s.u[i] = 0.0;
        s.col4row[i] = -1;
    }
    for (int j = lane; j < nc; j += 64) {
        s.v[j] = 0.0;
        s.row4col[j] = -1;
    }
    for (int cur = 0; cur < nr; ++cur) {
        for (int j = lane; j < nc; j += 64) {
            s.spc[j] = INFINITY;
            s.SC[j] = 0;
            s.remaining[j] = (short)(nc - 1 - j);
        }
        for (int i = lane; i < nr; i += 64) s.SR[i] = 0;
        __syncthreads();
        int num = nc, i = cur, sink = -1;  // uniform over the wavefront
        double minVal = 0.0;
        while (sink == -1) {
            if (lane == 0) s.SR[i] = 1;
            const double ui = s.u[i];
            LsapCand best{INFINITY, 0x7fffffff, false};
            for (int it = lane; it < num; it += 64) {
                const int j = s.remaining[it];
                const double r = ((minVal + cost(i, j)) - ui) - s.v[j];
                double sj = s.spc[j];
                if (r < sj) {
                    s.path[j] = (short)i;
                    s.spc[j] = r;
                    sj = r;
                }
                const LsapCand c{sj, it, s.row4col[j] < 0};
                if (lsap_better(c, best)) best = c;
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const LsapCand o{__shfl_xor(best.val, off, 64), __shfl_xor(best.pos, off, 64), __shfl_xor((int)best.open, off, 64) != 0};
                if (lsap_better(o, best)) best = o;
            }
            minVal = best.val;
            if (minVal == INFINITY) return 2;
            const int index = best.pos;
            const int j = s.remaining[index];
            const int r4 = s.row4col[j];
            if (r4 < 0)
                sink = j;
            else
                i = r4;
            --num;
            __syncthreads();  // every lane has read remaining[index]
            if (lane == 0) {
                s.SC[j] = 1;
                s.remaining[index] = s.remaining[num];
            }
            __syncthreads();
        }
        // dual updates (rows / columns of the tree), then the augmentation along path[]
        for (int r = lane; r < nr; r += 64)
            if (s.SR[r]) s.u[r] += r == cur ? minVal : minVal - s.spc[s.col4row[r]];
        for (int j = lane; j < nc; j += 64)
            if (s.SC[j]) s.v[j] -= minVal - s.spc[j];
        __syncthreads();
        if (lane == 0) {
            int j = sink;
            while (true) {
                const int r = s.path[j];
                s.row4col[j] = (short)r;
                const int t = s.col4row[r];
                s.col4row[r] = (short)j;
                j = t;
                if (r == cur) break;
            }
        }
        __syncthreads();
    }
    return 0;
}

}  // namespace shasta
