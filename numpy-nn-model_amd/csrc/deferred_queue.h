// deferred_queue.h -- the deferred-reduce queue of a kernel family (rowops.hip: RMSNorm / LayerNorm column sums; conv2d.hip: the
// reduces of a small-channel conv's weight-gradient partials).
// While parameter gradients are deferred (nnhipWeightGradDefer, common.h) a backward kernel writes its partials to the family's
// arena instead of the shared workspace and queues the reduce; the flush launches everything queued as ONE grid.  The arena is one
// per process: a StreamGuard (common.h) orders a reservation on another stream behind the last flush, and is held from the first
// reservation to the flush.
#pragma once
#include <mutex>

#include "common.h"

namespace nnhip {

// The group kernels find their job from start[]: job i owns blocks start[i] .. start[i+1]-1.  Unused slots repeat job 0 and own
// no block (start = the total).  Returns the grid size.
template <int MAX, class Job, class BlocksOf>
int group_starts(const Job* q, int n, Job* j, int* start, BlocksOf blocks_of) {
    int blocks = 0;
    for (int i = 0; i < MAX; ++i) {
        start[i] = blocks;
        j[i] = q[i < n ? i : 0];
        if (i < n) blocks += blocks_of(q[i]);
    }
    start[MAX] = blocks;
    return blocks;
}

template <class Job, int MAX>
class DeferredQueue {
public:
    // launches q[0..n) on st; `key` is what the family passed to reserve() for them
    using Launch = int (*)(const Job* q, int n, int key, hipStream_t st);
    explicit DeferredQueue(Launch launch) : launch_(launch) {}

    // `floats` of arena for `njobs` jobs the caller will push(), or nullptr: use the shared workspace and finish at once (*rc != 0:
    // an error).  What is queued is flushed first when it sits on another stream, was reserved under another `key` (jobs of one
    // launch share it), or leaves no room.  The arena grows to `grow_to` floats when it is too small -- nothing is queued then; never
    // while a captured graph holds the address.
    float* reserve(size_t floats, int njobs, int key, hipStream_t st, size_t grow_to, int* rc) {
        std::lock_guard<std::mutex> lk(mu_);
        *rc = 0;
        if (held_ && (st_ != st || key_ != key || n_ + njobs > MAX || used_ + floats > cap_)) *rc = flush_locked(st);
        if (*rc) return nullptr;
        if (floats > cap_ && !workspace_locked() && !stream_capturing(st)) {
            if (arena_) (void)hipFree(arena_);                // (synchronises: earlier reduces are done with it)
            arena_ = nullptr, cap_ = 0;
            if (hipMalloc(&arena_, grow_to * sizeof(float)) == hipSuccess) cap_ = grow_to;
            else arena_ = nullptr;
        }
        if (!arena_ || used_ + floats > cap_) return nullptr;
        if (!held_ && !(held_ = guard_.acquire(st))) {
            *rc = held_.rc;
            return nullptr;
        }
        float* p = arena_ + used_;
        used_ += (floats + 63) & ~(size_t)63;
        st_ = st;
        key_ = key;
        return p;
    }
    void push(const Job& job) {
        std::lock_guard<std::mutex> lk(mu_);
        q_[n_++] = job;
    }
    // launches what is queued, on the stream it was queued on; `stream` is the caller's
    int flush(hipStream_t stream) {
        std::lock_guard<std::mutex> lk(mu_);
        return flush_locked(stream);
    }
    void cleanup() {
        std::lock_guard<std::mutex> lk(mu_);
        n_ = 0;
        used_ = cap_ = 0;
        if (arena_) (void)hipFree(arena_);
        arena_ = nullptr;
        held_.done(false);
        guard_.reset();
    }

private:
    int flush_locked(hipStream_t callers) {
        const int n = n_;
        n_ = 0;
        used_ = 0;                                            // (a reservation whose launch failed leaves nothing queued: its floats come back too)
        const int rc = n ? launch_(q_, n, key_, st_) : 0;
        held_.done(st_ == callers);                           // (the queue's stream is a kept handle unless this caller passed it again)
        return rc;
    }
    Launch launch_;
    std::mutex mu_;
    Job q_[MAX];
    int n_ = 0, key_ = 0;
    hipStream_t st_ = nullptr;
    float* arena_ = nullptr;
    size_t cap_ = 0, used_ = 0;                               // floats
    StreamGuard guard_;
    StreamGuard::Use held_;
};

}  // namespace nnhip
