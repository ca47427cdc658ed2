// overlap.hip — hga_read_overlaps: approximate_read_overlap
// (src/clustering/ReadClusteringEngine.cpp:491-507) for a batch of read pairs on the lookup's
// device-resident first-occurrence lists (first_ptr / first_kid / first_pos).
//
// The reference intersects the two reads' KmerID multisets and takes, over the shared KmerIDs, the
// spread max - min of their kmer_positions in either read.  Duplicates of a KmerID share one position,
// so the result depends only on the set of shared KmerIDs: the intersection of the two distinct,
// ascending first_kid lists.
//
// One wave per pair (lists hold up to several thousand KmerIDs, a few hundred on average): the lanes
// stride over the shorter list and binary-search the longer one, keep running min / max of both
// positions and a hit count, and the wave reduces them with shuffles.  The waves stride over the pairs
// on their own, without a workgroup barrier, so a long pair holds back only the wave that has it.
#include <climits>

#include "hga_internal.hpp"

namespace hga {
namespace {

constexpr uint64_t OV_CHUNK = 1ull << 22;   // pairs per launch (16 MiB per scratch array)

__global__ __launch_bounds__(256) void ov_wave(const uint64_t* __restrict__ fptr, const uint32_t* __restrict__ fkid,
                                               const uint32_t* __restrict__ fpos, const uint32_t* __restrict__ ex,
                                               const uint32_t* __restrict__ ey, uint32_t n, uint32_t first_id,
                                               int32_t* __restrict__ ov, uint32_t* __restrict__ sh) {
    const int lane = (int)(threadIdx.x & 63u);
    // the wave's index as a scalar: the pair loop then branches for all 64 lanes at once, and every
    // shuffle below runs with the whole wave active
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    const uint32_t waves = gridDim.x * 4u;
    for (uint32_t e = wave; e < n; e += waves) {
        const uint32_t rx = ex[e] - first_id, ry = ey[e] - first_id;   // validated on the host
        uint64_t a0 = fptr[rx], b0 = fptr[ry];
        uint32_t la = (uint32_t)(fptr[rx + 1] - a0), lb = (uint32_t)(fptr[ry + 1] - b0);
        if (la > lb) {   // a: the shorter list (the result is symmetric in the two reads)
            const uint64_t t0 = a0;
            a0 = b0;
            b0 = t0;
            const uint32_t tl = la;
            la = lb;
            lb = tl;
        }
        const uint32_t* __restrict__ A = fkid + a0;
        const uint32_t* __restrict__ B = fkid + b0;
        int cnt = 0, min_a = INT_MAX, max_a = INT_MIN, min_b = INT_MAX, max_b = INT_MIN;
        uint32_t lo = 0;   // a lane's KmerIDs ascend: each search starts where its last one ended
        for (uint32_t i = (uint32_t)lane; i < la; i += 64u) {
            const uint32_t kid = A[i];
            uint32_t hi = lb;
            while (lo < hi) {   // lower_bound(B, kid)
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (B[mid] < kid) lo = mid + 1;
                else hi = mid;
            }
            if (lo < lb && B[lo] == kid) {
                const int pa = (int)fpos[a0 + i], pb = (int)fpos[b0 + lo];
                ++cnt;
                min_a = min(min_a, pa);
                max_a = max(max_a, pa);
                min_b = min(min_b, pb);
                max_b = max(max_b, pb);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            cnt += __shfl_xor(cnt, o, 64);
            min_a = min(min_a, __shfl_xor(min_a, o, 64));
            max_a = max(max_a, __shfl_xor(max_a, o, 64));
            min_b = min(min_b, __shfl_xor(min_b, o, 64));
            max_b = max(max_b, __shfl_xor(max_b, o, 64));
        }
        if (lane == 0) {
            ov[e] = cnt ? max(max_a - min_a, max_b - min_b) : 0;
            sh[e] = (uint32_t)cnt;
        }
    }
}

}  // namespace

void read_overlaps(hga_ctx* c, const uint32_t* x, const uint32_t* y, uint64_t n, int32_t* overlap, uint32_t* shared) {
    auto& L = c->lookup;
    auto& S = c->overlap;
    HGA_REQUIRE(L.ran, HGA_ERR_STATE, "hga_lookup_run not called");
    if (n == 0) return;
    HGA_REQUIRE(x && y, HGA_ERR_INVALID, "null ReadID list with n > 0");
    const uint64_t first = L.first_read_id, nr = L.n_reads;
    for (uint64_t i = 0; i < n; ++i)   // before anything is launched
        HGA_REQUIRE(x[i] >= first && x[i] - first < nr && y[i] >= first && y[i] - first < nr, HGA_ERR_INVALID,
                    "ReadID outside the lookup's reads");
    if (L.firsts == 0) {   // no read has a hit: every list is empty
        if (overlap) std::memset(overlap, 0, n * sizeof(int32_t));
        if (shared) std::memset(shared, 0, n * sizeof(uint32_t));
        return;
    }
    const uint64_t cap = std::min(n, OV_CHUNK);
    uint32_t* dx = static_cast<uint32_t*>(S.x.ensure(cap * 4));
    uint32_t* dy = static_cast<uint32_t*>(S.y.ensure(cap * 4));
    int32_t* dov = static_cast<int32_t*>(S.ov.ensure(cap * 4));
    uint32_t* dsh = static_cast<uint32_t*>(S.sh.ensure(cap * 4));
    for (uint64_t at = 0; at < n; at += OV_CHUNK) {
        const uint64_t m = std::min(OV_CHUNK, n - at);
        HGA_HIP(hipMemcpyAsync(dx, x + at, m * 4, hipMemcpyHostToDevice, c->stream));
        HGA_HIP(hipMemcpyAsync(dy, y + at, m * 4, hipMemcpyHostToDevice, c->stream));
        const unsigned grid = (unsigned)std::min<uint64_t>((m + 3) / 4, (uint64_t)c->num_cu * 8);
        c->launch("ov_wave", [&] {
            hipLaunchKernelGGL(ov_wave, dim3(grid), dim3(256), 0, c->stream, L.first_ptr.as<uint64_t>(),
                               L.first_kid.as<uint32_t>(), L.first_pos.as<uint32_t>(), dx, dy, (uint32_t)m,
                               L.first_read_id, dov, dsh);
        });
        c->check_launch("ov_wave");
        if (overlap) HGA_HIP(hipMemcpyAsync(overlap + at, dov, m * 4, hipMemcpyDeviceToHost, c->stream));
        if (shared) HGA_HIP(hipMemcpyAsync(shared + at, dsh, m * 4, hipMemcpyDeviceToHost, c->stream));
        c->sync();   // the scratch is reused by the next chunk
    }
}

}  // namespace hga
