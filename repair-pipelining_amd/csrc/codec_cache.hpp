// codec_cache.hpp -- the three caches behind the C ABI (ecx_api.cpp): the
// reference-counted registry of shared codecs (and the bundle of references one owner holds on
// it), the least-recently-used cache of per-call plans, and the build-once table of a codec's maps.
//
// Standard library only -- no HIP header, no ABI type, no unit of the engine: what they own is a
// template argument, so their counting, ordering and locking run -- and are tested -- on the CPU
// (tests/native/api_core_check.cpp, also under AddressSanitizer and ThreadSanitizer).
#pragma once

#include <cstddef>
#include <list>
#include <map>
#include <memory>
#include <mutex>
#include <unordered_map>
#include <vector>

namespace ecx {

// Equal keys are one reference-counted object.  get() takes a reference, release() drops it.  An
// object nobody references stays registered, idle, so that the next get() of its key finds it as
// it was left; at most `max_idle` idle objects are kept, least recently released first out.  Past
// `max_registered` registered objects, get() returns private objects that release() frees at once.
// Evicted and private objects are destroyed after the lock is released: a destructor may take its
// time (device memory) or come back to the registry.
template <typename T, typename Key>
class RefRegistry {
public:
    RefRegistry(size_t max_registered, size_t max_idle) : max_registered_(max_registered), max_idle_(max_idle) {}

    // The object of `key`, revived if it was idle, else `make()`'s -- a `new T`, built under the
    // lock; a throw registers nothing.
    template <typename Make>
    T *get(const Key &key, Make make) {
        std::lock_guard<std::mutex> lk(mu_);
        auto it = by_key_.find(key);
        if (it != by_key_.end()) {
            Record &r = *it->second;
            if (r.idle_at != idle_.end()) {
                idle_.erase(r.idle_at);
                r.idle_at = idle_.end();
            }
            ++r.refs;
            return r.obj.get();
        }
        std::unique_ptr<T> obj(make());
        T *p = obj.get();
        Record &r = by_ptr_[p];
        r.obj = std::move(obj);
        r.refs = 1;
        r.idle_at = idle_.end();
        r.key = by_key_.end();  // private, unless there is room:
        if (by_key_.size() < max_registered_) r.key = by_key_.emplace(key, &r).first;
        return p;
    }

    // Drops one reference; frees a private object, parks a shared one as idle when its last
    // reference goes.  Null, and a pointer the registry holds no live reference for (a second
    // release, a pointer it never issued), are ignored and never dereferenced.
    void release(T *obj) {
        if (!obj) return;
        std::vector<std::unique_ptr<T>> dead;  // outlives the lock
        std::lock_guard<std::mutex> lk(mu_);
        auto it = by_ptr_.find(obj);
        if (it == by_ptr_.end() || it->second.refs <= 0) return;
        Record &r = it->second;
        if (r.key == by_key_.end()) {
            dead.push_back(std::move(r.obj));
            by_ptr_.erase(it);
            return;
        }
        if (--r.refs > 0) return;
        idle_.push_front(&r);
        r.idle_at = idle_.begin();
        while (idle_.size() > max_idle_) {
            Record *victim = idle_.back();
            idle_.pop_back();
            by_key_.erase(victim->key);
            dead.push_back(std::move(victim->obj));
            by_ptr_.erase(dead.back().get());
        }
    }

    // Registered objects with a reference, and without.
    void stats(int *live, int *idle) {
        std::lock_guard<std::mutex> lk(mu_);
        if (live) *live = (int)(by_key_.size() - idle_.size());
        if (idle) *idle = (int)idle_.size();
    }

private:
    struct Record;
    using KeyIndex = std::map<Key, Record *>;
    struct Record {
        std::unique_ptr<T> obj;
        int refs = 0;
        typename KeyIndex::iterator key;                // by_key_.end(): private
        typename std::list<Record *>::iterator idle_at;  // idle_.end(): not idle
    };
    const size_t max_registered_, max_idle_;
    std::mutex mu_;
    std::map<const T *, Record> by_ptr_;  // owns the records
    KeyIndex by_key_;
    std::list<Record *> idle_;  // front = most recently released
};

// The references one owner holds on a registry's objects, one per distinct key (a Clay pattern
// set: one codec per distinct erased-node list).  get() takes a reference the first time a key is
// asked for and returns the same object afterwards; the destructor drops them all.
template <typename T, typename Key>
class RefBundle {
public:
    explicit RefBundle(RefRegistry<T, Key> &reg) : reg_(reg) {}
    ~RefBundle() {
        for (auto &kv : held_) reg_.release(kv.second);
    }
    RefBundle(const RefBundle &) = delete;
    RefBundle &operator=(const RefBundle &) = delete;
    template <typename Make>
    T *get(const Key &key, Make make) {
        auto it = held_.find(key);
        if (it != held_.end()) return it->second;
        T *obj = reg_.get(key, make);
        try {
            held_.emplace(key, obj);
        } catch (...) {
            reg_.release(obj);
            throw;
        }
        return obj;
    }
    size_t size() const { return held_.size(); }

private:
    RefRegistry<T, Key> &reg_;
    std::map<Key, T *> held_;
};

// Values by key, least recently used first out.  The capacity comes with each call (a knob the
// caller may change at any time).
template <typename Key, typename V>
class LruCache {
public:
    // The value of `key`, now the most recently used; on a miss `make()`'s (a shared_ptr), built
    // outside the lock -- where another thread built the same key meanwhile, that one is returned
    // and this one dropped.  Then the least recently used entries beyond `cap` leave; a value a
    // caller still holds lives until it lets go.  cap 0 builds every time and keeps nothing.
    template <typename Make>
    std::shared_ptr<V> get(const Key &key, size_t cap, Make make) {
        if (cap == 0) return make();
        {
            std::lock_guard<std::mutex> lk(mu_);
            auto it = index_.find(key);
            if (it != index_.end()) {
                lru_.splice(lru_.begin(), lru_, it->second);
                return it->second->second;
            }
        }
        std::shared_ptr<V> value = make();
        std::vector<std::shared_ptr<V>> evicted;  // outlives the lock
        std::lock_guard<std::mutex> lk(mu_);
        auto it = index_.find(key);
        if (it != index_.end()) return it->second->second;
        lru_.emplace_front(key, value);
        index_[key] = lru_.begin();
        while (lru_.size() > cap) {
            index_.erase(lru_.back().first);
            evicted.push_back(std::move(lru_.back().second));
            lru_.pop_back();
        }
        return value;
    }

    size_t size() {
        std::lock_guard<std::mutex> lk(mu_);
        return lru_.size();
    }

private:
    using Entry = std::pair<Key, std::shared_ptr<V>>;
    std::mutex mu_;
    std::list<Entry> lru_;  // front = most recently used
    std::unordered_map<Key, typename std::list<Entry>::iterator> index_;
};

// Values built once per key and kept as long as the table: get() returns the value of `key`,
// constructed from `make()`'s result under the lock if it is not there yet (a throw leaves the
// key without one).  The pointer stays valid as long as the Memo does.
template <typename Key, typename V>
class Memo {
public:
    template <typename Make>
    V *get(const Key &key, Make make) {
        std::lock_guard<std::mutex> lk(mu_);
        std::unique_ptr<V> &slot = values_[key];
        if (!slot) slot = std::make_unique<V>(make());
        return slot.get();
    }

private:
    std::mutex mu_;
    std::map<Key, std::unique_ptr<V>> values_;
};

}  // namespace ecx
