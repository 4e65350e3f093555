// table_cache.h -- the one cache of device-resident tables (NTT plans, the Plonk / Plookup circuit-size tables, the geometric and z_H
// tables of poly.hip), as plain C++: no HIP type in it, so that tests/table_cache_host.cpp runs the same code on the host, under
// ThreadSanitizer too.
//
// The rule, written once:
//  * get() holds the cache's own lock from the lookup to the insertion: two threads that ask for the same new key build it once, the
//    second one finds it.  A hit returns the stored pointer.  A miss constructs a T and runs build(T&) on it; the T is inserted only when
//    build returns PLK_OK - otherwise nothing is inserted, the half-built T is destroyed (its members free what they own) and the rc
//    passes through unchanged.
//  * A bounded cache (max_entries > 0) that is full drops the entry with the SMALLEST key before it inserts.
//  * clear() drops the cache's references.  The tables are handed out as shared_ptr: one still held by a running call lives until that
//    call lets go, and its destructor frees the buffers then (hipFree waits for kernels in flight).
//  * A build may call get() on ANOTHER cache (the Plonk and Plookup builds take the NTT plan's power table): the lock order is the
//    calling cache, then the called one, and must not form a cycle.
//  * Every cache enrols itself in a process-wide list; table_caches_clear() clears them all, one cache lock at a time and never while it
//    holds the list's lock (a build, under its cache's lock, may construct - and so enrol - another cache).  A new cache needs no edit
//    anywhere else to be cleared.
// Caches are meant to be file-static objects.  A cache leaves the list only at the end of its destruction, after its map and lock have
// gone: no cache may be destroyed while another thread may be in table_caches_clear() - one with a shorter life (a test's), and
// equally the file-static ones at process exit, when no thread may still be inside plk_ntt_clear_cache.
#pragma once
#include <algorithm>
#include <cstddef>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "../../include/plonky_hip.h"

namespace plk {

inline void table_caches_clear();  // clear() on every enrolled cache

class TableCacheBase {
  public:
    virtual void clear() = 0;
    TableCacheBase(const TableCacheBase&) = delete;
    TableCacheBase& operator=(const TableCacheBase&) = delete;

  protected:
    struct List {
        std::mutex mu;
        std::vector<TableCacheBase*> caches;
    };
    // a function-local static: there before the first file-scope cache enrols, whatever the initialisation order, and destroyed after
    // the last of them
    static List& list() {
        static List l;
        return l;
    }
    TableCacheBase() {
        List& l = list();
        std::lock_guard<std::mutex> lk(l.mu);
        l.caches.push_back(this);
    }
    ~TableCacheBase() {
        List& l = list();
        std::lock_guard<std::mutex> lk(l.mu);
        l.caches.erase(std::remove(l.caches.begin(), l.caches.end(), this), l.caches.end());
    }
    friend void table_caches_clear();
};

inline void table_caches_clear() {
    std::vector<TableCacheBase*> caches;
    {
        TableCacheBase::List& l = TableCacheBase::list();
        std::lock_guard<std::mutex> lk(l.mu);
        caches = l.caches;
    }
    for (TableCacheBase* c : caches) c->clear();
}

template <class Key, class T>
class TableCache final : public TableCacheBase {
    std::mutex mu_;
    std::map<Key, std::shared_ptr<T>> map_;
    const size_t max_entries_;

  public:
    explicit TableCache(size_t max_entries = 0) : max_entries_(max_entries) {}  // 0: unbounded

    template <class Build>  // int(T&): PLK_OK on success
    int get(const Key& key, std::shared_ptr<T>& out, Build&& build) {
        std::lock_guard<std::mutex> lk(mu_);
        auto it = map_.find(key);
        if (it != map_.end()) {
            out = it->second;
            return PLK_OK;
        }
        auto t = std::make_shared<T>();
        const int rc = build(*t);
        if (rc != PLK_OK) return rc;
        if (max_entries_ && map_.size() >= max_entries_) map_.erase(map_.begin());
        map_[key] = t;
        out = std::move(t);
        return PLK_OK;
    }

    void clear() override {
        std::lock_guard<std::mutex> lk(mu_);
        map_.clear();
    }
};

}  // namespace plk
