// flink_kg_format.h — host-side codec of one key group of a Flink 1.2 WindowOperator checkpoint
// (SURVEY.md §8f.1), used by fw_snapshot_kg_flink / fw_restore_kg_flink.
//
//   state   what HeapKeyedStateBackend.snapshot writes at KeyGroupRangeOffsets[kg]
//           (flink-runtime/.../state/heap/HeapKeyedStateBackend.java:196-212, writeStateTableForKeyGroup
//           :217-248): int kg | short state id (0: "window-contents" is the operator's only keyed state,
//           WindowOperator.java:310-311) | byte present | int numNamespaces |
//           (TimeWindow: long start, long end (TimeWindow.Serializer, TimeWindow.java:141-144) |
//            int numEntries | (key, state tuple)*)*
//   timers  HeapInternalTimerService.snapshotTimersForKeyGroup (SJ/api/operators/HeapInternalTimerService.java
//           :285-310) after its two serializeObject records: int n | (key | start | end | long timestamp)*
//           (InternalTimer.TimerSerializer.serialize, InternalTimer.java:145-149) | int 0 processing timers
//
// Everything is big-endian (DataOutputStream).  Keys are Long / Tuple1<Long> (LongSerializer, 8 bytes);
// state tuple fields are LongSerializer / DoubleSerializer values (writeDouble = doubleToLongBits: one
// canonical NaN), in TupleSerializer field order (TupleSerializer.java:120-129).
//
// Iteration order.  The namespaces of a key group, the entries of a namespace and the timers of a key
// group live in java.util.HashMap / HashSet: iteration goes bucket by bucket, bucket = spread(hashCode) &
// (capacity - 1) with spread(h) = h ^ (h >>> 16), and within a bucket in insertion order (puts append to
// the bin's chain; a resize splits a chain without reordering it).  The capacity is 16, doubled while
// size > 3/4 capacity.  A JVM table never shrinks, so its capacity reflects the largest size it ever had;
// the codec sizes it by the current size (the two agree unless the table once held more entries, e.g. a
// timer set right before a watermark fired part of it).  Chains longer than 8 in a table of >= 64
// buckets become red-black trees in the JVM with a different order; not emulated.
//
// Host-only (no HIP, no engine types; tests/sanitize/host_sanitize.cpp drives it under ASan/UBSan).  Above the
// bytes (BeOut / BeIn, the hashes, hashmap_order) sits the section codec — the timer section, the "window-contents"
// table, the copy-out: framing, HashMap order and the checks that need no meaning (counts, truncation, a key field
// that differs from its entry's key).  Values cross it as raw 8-byte words; what a word means (double min/max codes,
// fold, the namespaces an assigner allows, key groups, duplicates) is the caller's, whom the reader hands each
// namespace and entry as it meets them, so that the caller's checks fail in blob order.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <map>
#include <utility>
#include <vector>

#include "../../include/flink_window.h"
#include "java_semantics.h"

namespace fwkg {

struct BeOut {
  std::vector<uint8_t> b;
  void u8(uint32_t v) { b.push_back((uint8_t)v); }
  void i16(int32_t v) { u8((uint32_t)v >> 8); u8((uint32_t)v); }
  void i32(int32_t v) { for (int s = 24; s >= 0; s -= 8) u8((uint32_t)v >> s); }
  void i64(int64_t v) { for (int s = 56; s >= 0; s -= 8) u8((uint32_t)((uint64_t)v >> s)); }
  void f64(double d) {   // DataOutputStream.writeDouble: writeLong(Double.doubleToLongBits(d))
    int64_t x;
    if (d != d) x = 0x7ff8000000000000ll;
    else memcpy(&x, &d, 8);
    i64(x);
  }
};

struct BeIn {
  const uint8_t* p;
  int64_t n, pos = 0;
  bool ok = true;
  BeIn(const void* d, int64_t len) : p((const uint8_t*)d), n(len) {}
  uint64_t take(int k) {
    if (!ok || pos + k > n) { ok = false; return 0; }
    uint64_t v = 0;
    for (int i = 0; i < k; ++i) v = (v << 8) | p[pos + i];
    pos += k;
    return v;
  }
  int32_t u8() { return (int32_t)take(1); }
  int32_t i16() { return (int32_t)(int16_t)take(2); }
  int32_t i32() { return (int32_t)take(4); }
  int64_t i64() { return (int64_t)take(8); }
  bool done() const { return ok && pos == n; }
};

// java.util.HashMap.hash(key) and the table capacity for `n` entries put into a new HashMap()
inline int32_t spread(int32_t h) { return (int32_t)((uint32_t)h ^ ((uint32_t)h >> 16)); }
inline uint32_t capacity_for(size_t n) {
  uint64_t c = 16;
  while (n > c / 4 * 3) c <<= 1;
  return (uint32_t)c;
}
inline int32_t jmul31(int32_t a) { return (int32_t)((uint32_t)a * 31u); }
inline int32_t jaddi(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
// TimeWindow.hashCode (TimeWindow.java:79-83)
inline int32_t window_hash(int64_t start, int64_t end) {
  return jaddi(jmul31(fw::long_hash_code(start)), fw::long_hash_code(end));
}
// InternalTimer.hashCode (InternalTimer.java:81-86) with key.hashCode = Long.hashCode
inline int32_t timer_hash(int64_t ts, int64_t key, int64_t start, int64_t end) {
  int32_t r = fw::long_hash_code(ts);
  r = jaddi(jmul31(r), fw::long_hash_code(key));
  return jaddi(jmul31(r), window_hash(start, end));
}

// Sort `idx` into HashMap iteration order: bucket of hash(i), then insertion rank(i) (a strict order).
template <class Hash, class Less>
void hashmap_order(std::vector<size_t>& idx, Hash hash, Less earlier) {
  const uint32_t mask = capacity_for(idx.size()) - 1;
  std::sort(idx.begin(), idx.end(), [&](size_t a, size_t b) {
    const uint32_t ba = (uint32_t)spread(hash(a)) & mask, bb = (uint32_t)spread(hash(b)) & mask;
    if (ba != bb) return ba < bb;
    return earlier(a, b);
  });
}

// ---- timer section: int n | (key | start | end | long timestamp)* | int 0 processing-time timers ----

struct Timer {
  int64_t key, start, end, ts;
  std::array<int64_t, 4> tie() const { return {key, start, end, ts}; }
  bool operator<(const Timer& o) const { return tie() < o.tie(); }
  bool operator==(const Timer& o) const { return tie() == o.tie(); }
};

// `n` timers (at(i)) as the JVM's HashSet<InternalTimer> iterates them: bucket of timer_hash, then insertion
// order — restored timers first, in their blob order (restored_rank: Timer -> rank, empty when nothing was
// restored), then the caller's `earlier(i, j)` among the rest
template <class At, class Earlier>
std::vector<Timer> timers_in_set_order(size_t n, At at, const std::map<Timer, int64_t>& restored_rank, Earlier earlier) {
  std::vector<Timer> t(n);
  std::vector<int64_t> rank(n, INT64_MAX);
  std::vector<size_t> idx(n);
  for (size_t i = 0; i < n; ++i) {
    t[i] = at(i);
    idx[i] = i;
    auto it = restored_rank.find(t[i]);
    if (it != restored_rank.end()) rank[i] = it->second;
  }
  hashmap_order(
      idx, [&](size_t i) { return timer_hash(t[i].ts, t[i].key, t[i].start, t[i].end); },
      [&](size_t a, size_t b) { return rank[a] != rank[b] ? rank[a] < rank[b] : earlier(a, b); });
  std::vector<Timer> out;
  out.reserve(n);
  for (size_t i : idx) out.push_back(t[i]);
  return out;
}

inline void write_timers(BeOut& o, const std::vector<Timer>& ordered) {
  o.i32((int32_t)ordered.size());
  for (const Timer& t : ordered) { o.i64(t.key); o.i64(t.start); o.i64(t.end); o.i64(t.ts); }
  o.i32(0);
}

enum class TimersFail { none, negative_count, truncated_or_trailing, processing_timers };

// the timers in blob order; on a failure `out` holds the ones read so far
inline TimersFail read_timers(const void* section, int64_t len, std::vector<Timer>& out) {
  BeIn in(section, len);
  out.clear();
  const int32_t n = in.i32();
  if (n < 0) return TimersFail::negative_count;
  for (int32_t i = 0; i < n && in.ok; ++i) {
    Timer t;
    t.key = in.i64(); t.start = in.i64(); t.end = in.i64(); t.ts = in.i64();
    if (in.ok) out.push_back(t);
  }
  const int32_t np = in.i32();
  if (!in.done()) return TimersFail::truncated_or_trailing;
  return np != 0 ? TimersFail::processing_timers : TimersFail::none;
}

// ---- "window-contents" state table (after `int kg | short id | byte present`):
//      int numNamespaces | (long start, long end | int numEntries | (key | value)*)*
//      value: the layout's fields (reducing / folding state), or ListSerializer's int size | element* with the
//      layout's fields per element (list state) ----

struct WcLayout { const int32_t* field; int32_t n_fields; bool list; };   // field: FW_SF_* in serializer order

// one entry's value as raw big-endian words (a double: its doubleToLongBits, see double_word)
struct WcEntry {
  int64_t key = 0;
  std::vector<int64_t> word;                   // reducing state: one per layout field (FW_SF_KEY's slot: the key)
  std::vector<std::array<int64_t, 2>> el;      // list state: (FW_SF_VALUE, FW_SF_F1) of each element, in list order
};

// DataOutputStream.writeDouble's word for a double held as bits: doubleToLongBits (one canonical NaN)
inline int64_t double_word(int64_t bits) {
  const uint64_t u = (uint64_t)bits & 0x7fffffffffffffffull;
  return u > 0x7ff0000000000000ull ? 0x7ff8000000000000ll : bits;
}

struct WcNamespace { int64_t start, end; std::vector<size_t> entries; };   // entries: the caller's entry ids

// entries 0 .. n-1 grouped by namespace(i) = (start, end): namespaces ascending, each one's entries ascending
template <class NamespaceOf>
std::vector<WcNamespace> group_namespaces(size_t n, NamespaceOf namespace_of) {
  std::map<std::pair<int64_t, int64_t>, std::vector<size_t>> m;
  for (size_t i = 0; i < n; ++i) m[namespace_of(i)].push_back(i);
  std::vector<WcNamespace> out;
  for (auto& kv : m) out.push_back({kv.first.first, kv.first.second, std::move(kv.second)});
  return out;
}

// The table in the JVM's order: namespaces by TimeWindow.hashCode then ns_earlier(a, b) (indices into `ns`),
// a namespace's entries by Long.hashCode(key_of(id)) then entry_earlier(id, id).  fill(id, entry) supplies the
// value words (entry.key is set; word / el arrive empty)
template <class NsEarlier, class KeyOf, class EntryEarlier, class Fill>
void write_window_contents(BeOut& o, const WcLayout& L, std::vector<WcNamespace>& ns, NsEarlier ns_earlier, KeyOf key_of,
                           EntryEarlier entry_earlier, Fill fill) {
  std::vector<size_t> order(ns.size());
  for (size_t w = 0; w < order.size(); ++w) order[w] = w;
  hashmap_order(order, [&](size_t w) { return window_hash(ns[w].start, ns[w].end); }, ns_earlier);
  o.i32((int32_t)ns.size());
  WcEntry ent;
  for (size_t w : order) {
    o.i64(ns[w].start); o.i64(ns[w].end);
    std::vector<size_t>& ids = ns[w].entries;
    hashmap_order(ids, [&](size_t i) { return fw::long_hash_code(key_of(i)); }, entry_earlier);
    o.i32((int32_t)ids.size());
    for (size_t i : ids) {
      ent.key = key_of(i); ent.word.clear(); ent.el.clear();
      fill(i, ent);
      o.i64(ent.key);
      for (int f = 0; f < L.n_fields && !L.list; ++f) o.i64(ent.word[(size_t)f]);
      if (L.list) o.i32((int32_t)ent.el.size());
      for (const auto& x : ent.el)
        for (int f = 0; f < L.n_fields; ++f)
          o.i64(L.field[f] == FW_SF_KEY ? ent.key : L.field[f] == FW_SF_F1 ? x[1] : x[0]);
    }
  }
}

// stopped: a callback returned false (the caller holds the reason); negative_count: of namespaces or entries;
// entry / element_key_differs: the FW_SF_KEY field of a reducing state / of a list element is not the entry's key
enum class WcFail { none, stopped, truncated, negative_count, negative_list_size, empty_list, entry_key_differs,
                    element_key_differs };

// Reads the table at `in`, in blob order: on_namespace(start, end) before the namespace's entries,
// on_entry(start, end, entry) after each complete entry; either returns false to stop
template <class OnNamespace, class OnEntry>
WcFail read_window_contents(BeIn& in, const WcLayout& L, OnNamespace on_namespace, OnEntry on_entry) {
  const int32_t nns = in.i32();
  if (nns < 0) return WcFail::negative_count;
  WcEntry ent;
  for (int32_t w = 0; w < nns && in.ok; ++w) {
    const int64_t start = in.i64(), end = in.i64();
    if (in.ok && !on_namespace(start, end)) return WcFail::stopped;
    const int32_t ne = in.i32();
    if (ne < 0) return WcFail::negative_count;
    for (int32_t j = 0; j < ne && in.ok; ++j) {
      ent.key = in.i64(); ent.word.clear(); ent.el.clear();
      int32_t nel = 1;   // (reducing state: one tuple of the layout's fields; list state: int size, then one per element)
      if (L.list && (nel = in.i32()) < 0) return WcFail::negative_list_size;
      for (int32_t q = 0; q < nel && in.ok; ++q) {
        std::array<int64_t, 2> x{0, 0};
        for (int f = 0; f < L.n_fields; ++f) {
          const int64_t v = in.i64();
          if (L.field[f] == FW_SF_KEY && in.ok && v != ent.key) return L.list ? WcFail::element_key_differs : WcFail::entry_key_differs;
          if (!L.list) ent.word.push_back(v);
          else if (L.field[f] == FW_SF_F1) x[1] = v;
          else if (L.field[f] == FW_SF_VALUE) x[0] = v;
        }
        if (L.list) ent.el.push_back(x);
      }
      if (in.ok && L.list && ent.el.empty()) return WcFail::empty_list;
      if (in.ok && !on_entry(start, end, ent)) return WcFail::stopped;
    }
  }
  return in.ok ? WcFail::none : WcFail::truncated;
}

// ---- copy-out of both sections; both buffers null: the lengths only.  False: a buffer missing or too small ----
inline bool copy_sections(const BeOut& state, const BeOut& timers, void* state_buf, int64_t state_cap, int64_t* state_len,
                          void* timers_buf, int64_t timers_cap, int64_t* timers_len) {
  *state_len = (int64_t)state.b.size();
  *timers_len = (int64_t)timers.b.size();
  if (!state_buf && !timers_buf) return true;
  if (!state_buf || !timers_buf || state_cap < *state_len || timers_cap < *timers_len) return false;
  if (!state.b.empty()) memcpy(state_buf, state.b.data(), state.b.size());
  if (!timers.b.empty()) memcpy(timers_buf, timers.b.data(), timers.b.size());
  return true;
}

}  // namespace fwkg
