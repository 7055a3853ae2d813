// plans.hpp — the plans a handle keeps between calls: what each training forward laid out in its workspace, keyed by the
// workspace address, until the backward of that forward has read it.  Host code only (no HIP include): net.hip uses it
// with its Plan, tests/host/plans_main.cpp with an int.
//
// The contract (include/unet_hip.h states it for callers):
//   * remember(key): the entry is PENDING, and the newest.  A key that is already present is replaced.
//   * finish(key):   the last backward stage of that forward has been enqueued once; the entry is FINISHED.  It stays
//                    readable (a backward may be repeated) until it is evicted.
//   * eviction:      finished entries leave, the one finished longest ago first, once more than FINISHED_KEPT of them exist
//                    (so the entry that has just been finished is never the one to go).  A pending
//                    entry is never evicted to make room for another: its caller still holds a live workspace, so their
//                    number is bounded by device memory.
//   * PENDING_MAX:   the one hard bound, against callers that abandon training forwards (never run their backward, never
//                    reuse the address): past it the oldest pending entry is dropped.  A Plan is about 1.5 KB, so a handle
//                    keeps at most ~1.6 MB of them.
//   * forget(key):   the entry is gone (an inference forward has overwritten that workspace).
// Every method takes the registry's own mutex.
#pragma once

#include <cstddef>
#include <mutex>
#include <vector>

namespace unet {

template <class T>
class PlanRegistry {
public:
    static constexpr size_t FINISHED_KEPT = 16;
    static constexpr size_t PENDING_MAX = 1024;

    void remember(const void *key, const T &value)
    {
        std::lock_guard<std::mutex> lk(mu_);
        erase_key(key);
        if (count(true) >= PENDING_MAX) erase_oldest(true);
        entries_.push_back(Entry{key, true, value});
    }

    // the plan at `key`, pending or finished
    bool lookup(const void *key, T &value) const
    {
        std::lock_guard<std::mutex> lk(mu_);
        for (const Entry &e : entries_)
            if (e.key == key) { value = e.value; return true; }
        return false;
    }

    // pending -> finished (finishing twice is harmless); false when the key is not present
    bool finish(const void *key)
    {
        std::lock_guard<std::mutex> lk(mu_);
        size_t i = 0;
        while (i < entries_.size() && entries_[i].key != key) ++i;
        if (i == entries_.size()) return false;
        Entry e = entries_[i];
        e.pending = false;
        entries_.erase(entries_.begin() + i);
        entries_.push_back(e);           // the newest of the finished: whoever finished it may still read it (unet_backward_input)
        while (count(false) > FINISHED_KEPT) erase_oldest(false);
        return true;
    }

    bool forget(const void *key)
    {
        std::lock_guard<std::mutex> lk(mu_);
        return erase_key(key);
    }

    bool pending(const void *key) const
    {
        std::lock_guard<std::mutex> lk(mu_);
        for (const Entry &e : entries_)
            if (e.key == key) return e.pending;
        return false;
    }
    size_t size() const { std::lock_guard<std::mutex> lk(mu_); return entries_.size(); }
    size_t pending_count() const { std::lock_guard<std::mutex> lk(mu_); return count(true); }

private:
    struct Entry { const void *key; bool pending; T value; };
    mutable std::mutex mu_;
    std::vector<Entry> entries_;         // in the order of their last remember() / finish(), oldest first

    size_t count(bool pending) const
    {
        size_t n = 0;
        for (const Entry &e : entries_) n += e.pending == pending;
        return n;
    }
    bool erase_key(const void *key)
    {
        for (size_t i = 0; i < entries_.size(); ++i)
            if (entries_[i].key == key) { entries_.erase(entries_.begin() + i); return true; }
        return false;
    }
    void erase_oldest(bool pending)
    {
        for (size_t i = 0; i < entries_.size(); ++i)
            if (entries_[i].pending == pending) { entries_.erase(entries_.begin() + i); return; }
    }
};

}  // namespace unet
