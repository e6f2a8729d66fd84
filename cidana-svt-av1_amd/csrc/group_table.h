// group_table.h — the group table of the whole-picture launches, written once for the device and for the host.
//
// A launch covers the workgroups of all its groups back to back.  The table rides in the kernel arguments (no device-side
// descriptor memory: the call stays a pure enqueue and is graph-capturable, and it has to fit their 4 KiB: keep a
// static_assert(sizeof(Desc) <= 4000) next to every descriptor).  A descriptor is
//     struct Desc { int32_t ngroups; ...launch-wide fields...; Group g[MAX]; };      Group has a member  uint32_t wg_end;
// and group i owns the workgroups [g[i - 1].wg_end, g[i].wg_end): wg_end is one past the group's last workgroup, nothing else.
#pragma once
#include <stdint.h>
#include <type_traits>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
namespace svtdev {
// Returns the group of workgroup blockIdx.x (fd.ngroups when past the last) and its index bid inside that group.  Uniform: scalar
// compares against the table.  (cfl_frame_kernel, kernel_cfl.h, spells the loop out: see there.)
template <typename Desc>
__device__ __forceinline__ int group_of(const Desc& fd, uint32_t& bid) {
    int gi = 0;
    uint32_t start = 0;
#pragma unroll 1
    for (int i = 0; i < fd.ngroups; i++) {
        if (blockIdx.x >= fd.g[i].wg_end) { gi = i + 1; start = fd.g[i].wg_end; }
    }
    bid = blockIdx.x - start;
    return gi;
}
}  // namespace svtdev
#endif

// ---- host: plain C++17, no HIP header, so that a CPU program can include it (tests/c/group_table_host.cpp) ----
namespace svthost {

constexpr uint32_t kMaxLaunchWgs = 0x7fffffffu;           // workgroups of one launch
constexpr int kGroupTooLarge = -2;                        // (SVT_HIP_ERR_INVALID: host_common.h asserts it)

// order[0 .. n) = the indices 0 .. n - 1 by key(i) descending, equal keys in index order (a stable insertion sort: n is small).
// "Largest first": the long workgroups, or the long kernels, start early and the short ones fill in beside them.
template <typename Key>
inline void order_largest_first(int* order, int n, Key key) {
    for (int i = 0; i < n; i++) {
        int j = i - 1;
        while (j >= 0 && key(order[j]) < key(i)) { order[j + 1] = order[j]; j--; }
        order[j + 1] = i;
    }
}

// Builds a Desc group by group and hands it to launch(desc, total_workgroups) -> int (0 = OK) at flush().  A group's own workgroup
// count is kept beside the table; the running wg_end is computed in one place, at flush.  LARGEST_FIRST: flush orders the groups by
// the key given to add(), largest first.  desc's launch-wide fields are the caller's and survive a flush.
template <typename Desc, int MAX, bool LARGEST_FIRST = false>
class GroupTable {
    int n_ = 0;
    uint32_t total_ = 0, wgs_[MAX];
    uint64_t key_[LARGEST_FIRST ? MAX : 1];

public:
    using Group = std::remove_extent_t<decltype(Desc::g)>;
    static_assert(std::extent_v<decltype(Desc::g)> == MAX && std::is_trivially_copyable_v<Desc>, "Desc::g[MAX], passed by value");
    Desc desc{};
    int rc = 0;                                            // why the flushing add() returned null
    int size() const { return n_; }
    // no room for a group of wgs workgroups: no slot left, or the launch would pass kMaxLaunchWgs
    bool full(uint32_t wgs = 0) const { return n_ == MAX || (uint64_t)total_ + wgs > kMaxLaunchWgs; }
    // the next slot, zeroed, for a group of wgs workgroups; null when full(wgs).  For callers that must not launch mid-build.
    Group* add(uint32_t wgs, uint64_t key = 0) {
        if (full(wgs)) return nullptr;
        wgs_[n_] = wgs;
        key_[LARGEST_FIRST ? n_ : 0] = key;
        total_ += wgs;
        return &(desc.g[n_++] = Group{});
    }
    // the same, after flushing what the table holds if the group does not fit beside it.  Null: rc is that flush's error, or
    // kGroupTooLarge for a group that no launch holds.
    template <typename Launch>
    Group* add(uint32_t wgs, Launch&& launch, uint64_t key = 0) {
        rc = wgs > kMaxLaunchWgs ? kGroupTooLarge : (full(wgs) ? flush(launch) : 0);
        return rc ? nullptr : add(wgs, key);
    }
    // orders the groups, writes every wg_end, launches, and leaves the table empty.  An empty table launches nothing.
    template <typename Launch>
    int flush(Launch&& launch) {
        if (!n_) return 0;
        if constexpr (LARGEST_FIRST) {
            int order[MAX];
            order_largest_first(order, n_, [&](int i) { return key_[i]; });
            const GroupTable from = *this;
            for (int i = 0; i < n_; i++) { desc.g[i] = from.desc.g[order[i]]; wgs_[i] = from.wgs_[order[i]]; }
        }
        uint32_t total = 0;
        for (int i = 0; i < n_; i++) desc.g[i].wg_end = total += wgs_[i];
        desc.ngroups = n_;
        n_ = 0;
        total_ = 0;
        return launch(static_cast<const Desc&>(desc), total);
    }
};

}  // namespace svthost
