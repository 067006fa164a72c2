// Host-code sanitizer driver (-fsanitize=address,undefined on host code; GPU sanitizers are not
// available on the pool).  Built by tests/test_host_sanitizers.py with g++ -fsanitize=address,undefined
// -fno-sanitize-recover=all together with oracle/fw_oracle.cpp (the CPU parity oracle: test infrastructure)
// and run as a plain process.  It drives
//   - the oracle through every window shape the engine offers: tumbling / sliding / session, reduce (sum,
//     min, max, count, doubles), allowed lateness with both triggers, fold, list state, maxBy, the
//     checkpoint writer and reader of the reference's byte layout (every key group snapshotted, restored
//     into a fresh oracle, snapshotted again: identical bytes), and the wire-format decoder (whole and cut
//     streams, a corrupt tag);
//   - flink_kg_format.h, the engine's host-side checkpoint codec: big-endian writer / reader round trips,
//     reads past the end (ok = false), HashMap iteration order over random tables; its section layer: timer
//     sections and "window-contents" tables (reducing and list state) written, read and written back, every
//     strict prefix of a section in a buffer of exactly its size, corrupt counts and key fields, the copy-out.
// Any sanitizer report aborts with a non-zero status; the test asserts status 0.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/flink_window.h"
#include "../../flink_amd/csrc/flink_kg_format.h"

extern "C" {
int fwo_create(const fw_config* cfg, fw_engine** out);
int fwo_push_batch(fw_engine* e, const int64_t* key, const int32_t* key_hash, const int64_t* f1, const int64_t* ts,
                   const void* value, int64_t n);
int fwo_advance_watermark(fw_engine* e, int64_t wm);
int fwo_collect(fw_engine* e, fw_out* o);
int fwo_get_stats(fw_engine* e, fw_stats* st);
int fwo_snapshot_kg_flink(fw_engine* e, int32_t kg, const fw_state_layout* layout, void* state, int64_t state_cap,
                          int64_t* state_len, void* timers, int64_t timers_cap, int64_t* timers_len);
int fwo_restore_kg_flink(fw_engine* e, int32_t kg, const fw_state_layout* layout, int64_t watermark, const void* state,
                         int64_t state_len, const void* timers, int64_t timers_len);
int fwo_decode(fw_engine* e, const fw_tuple_schema* sc, const void* bytes, int64_t nbytes, int32_t mem, int64_t* key,
               int32_t* key_hash, int64_t* f1, int64_t* ts, void* value, int64_t record_cap, int64_t* wm,
               int64_t* wm_pos, int64_t* lm, int64_t* lm_pos, int64_t marker_cap, fw_decode_counts* out);
const char* fwo_last_error(const fw_engine* e);
void fwo_destroy(fw_engine* e);
}

static int failures = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

static uint64_t splitmix(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static fw_config base_config() {
  fw_config c;
  memset(&c, 0, sizeof(c));
  c.assigner = FW_TUMBLING;
  c.size = 1000;
  c.trigger = FW_TRIGGER_EVENT_TIME;
  c.value_type = FW_VALUE_I64;
  c.agg_mask = FW_AGG_SUM;
  c.keep_first_f1 = 1;
  c.max_parallelism = 128;
  c.kg_start = 0;
  c.kg_end = 127;
  c.key_capacity = 1 << 12;
  c.max_batch = 1 << 12;
  c.out_capacity = 1 << 18;
  return c;
}

// drive n records (keys < nk, ts advancing at rate per ms with out-of-order jitter) in batches, a watermark
// after each; returns fired records
static int64_t drive(fw_engine* e, int64_t n, int nk, int64_t t0, int ooo, bool f64, int64_t lag, uint64_t seed) {
  std::vector<int64_t> k(1024), t(1024), f1(1024), v(1024);
  int64_t fired = 0, max_ts = INT64_MIN;
  for (int64_t s = 0; s < n; s += 1024) {
    const int m = (int)std::min<int64_t>(1024, n - s);
    for (int i = 0; i < m; ++i) {
      const uint64_t r = splitmix(seed ^ (uint64_t)(s + i));
      k[i] = (int64_t)(r % (uint64_t)nk);
      t[i] = t0 + (s + i) / 8 - (ooo ? (int64_t)(splitmix(r) % (uint64_t)(ooo + 1)) : 0);
      f1[i] = (int64_t)r;
      if (f64) { double d = (double)(r >> 11) / 9007199254740992.0 - 0.25; memcpy(&v[i], &d, 8); }
      else v[i] = (int64_t)splitmix(r ^ 7);
      if (t[i] > max_ts) max_ts = t[i];
    }
    CHECK(fwo_push_batch(e, k.data(), nullptr, f1.data(), t.data(), v.data(), m) == FW_OK);
    CHECK(fwo_advance_watermark(e, max_ts - lag) == FW_OK);
    fw_out o;
    CHECK(fwo_collect(e, &o) == FW_OK);
    fired += o.n;
    for (int64_t i = 0; i < o.n; ++i) CHECK(o.key[i] >= 0 && o.key[i] < nk);
  }
  CHECK(fwo_advance_watermark(e, INT64_MAX) == FW_OK);
  fw_out o;
  CHECK(fwo_collect(e, &o) == FW_OK);
  return fired + o.n;
}

static void snapshot_restore_roundtrip(const fw_config& c, int64_t n, const fw_state_layout& L) {
  fw_engine* e = nullptr;
  CHECK(fwo_create(&c, &e) == FW_OK);
  // a run that leaves windows open: no final watermark
  std::vector<int64_t> k(n), t(n), v(n);
  for (int64_t i = 0; i < n; ++i) {
    const uint64_t r = splitmix(0xabc ^ (uint64_t)i);
    k[i] = (int64_t)(r % 500);
    t[i] = i / 4;
    v[i] = (int64_t)(r >> 3);
  }
  CHECK(fwo_push_batch(e, k.data(), nullptr, nullptr, t.data(), v.data(), n) == FW_OK);
  fw_engine* r = nullptr;
  CHECK(fwo_create(&c, &r) == FW_OK);
  for (int kg = 0; kg < c.max_parallelism; ++kg) {
    int64_t ns = 0, nt = 0;
    CHECK(fwo_snapshot_kg_flink(e, kg, &L, nullptr, 0, &ns, nullptr, 0, &nt) == FW_OK);
    std::vector<uint8_t> st((size_t)ns + 1), tm((size_t)nt + 1);
    CHECK(fwo_snapshot_kg_flink(e, kg, &L, st.data(), ns, &ns, tm.data(), nt, &nt) == FW_OK);
    if (ns == 0) continue;
    CHECK(fwo_restore_kg_flink(r, kg, &L, INT64_MIN, st.data(), ns, tm.data(), nt) == FW_OK);
    int64_t ns2 = 0, nt2 = 0;
    std::vector<uint8_t> st2((size_t)ns + 1), tm2((size_t)nt + 1);
    CHECK(fwo_snapshot_kg_flink(r, kg, &L, st2.data(), ns, &ns2, tm2.data(), nt, &nt2) == FW_OK);
    CHECK(ns2 == ns && nt2 == nt && memcmp(st.data(), st2.data(), (size_t)ns) == 0 &&
          memcmp(tm.data(), tm2.data(), (size_t)nt) == 0);
    // truncated blobs are rejected, never read past their end
    if (ns > 3) CHECK(fwo_restore_kg_flink(r, kg, &L, INT64_MIN, st.data(), ns - 3, tm.data(), nt) != FW_OK);
  }
  fwo_destroy(e);
  fwo_destroy(r);
}

static void decode_streams() {
  // Tuple3<Long, Long, Long> records with timestamps, a watermark, a latency marker
  std::vector<uint8_t> b;
  auto be = [&](uint64_t x, int nb) { for (int s = 8 * (nb - 1); s >= 0; s -= 8) b.push_back((uint8_t)(x >> s)); };
  for (int i = 0; i < 300; ++i) {
    be(33, 4); b.push_back(0); be((uint64_t)(1000 + i), 8);
    be((uint64_t)(i % 17), 8); be((uint64_t)(1000 + i), 8); be(splitmix((uint64_t)i), 8);
    if (i % 50 == 49) { be(9, 4); b.push_back(2); be((uint64_t)(1000 + i), 8); }
    if (i % 70 == 3) { be(17, 4); b.push_back(3); be(77, 8); be(5, 4); be(1, 4); }
  }
  fw_tuple_schema sc;
  memset(&sc, 0, sizeof(sc));
  sc.n_fields = 3;
  sc.key_field = 0;
  sc.f1_field = 1;
  sc.value_field = 2;
  std::vector<int64_t> key(400), f1(400), ts(400), val(400), wm(64), wmp(64), lm(128), lmp(64);
  fw_decode_counts cnt;
  for (int64_t cut : {(int64_t)b.size(), (int64_t)b.size() - 5, (int64_t)17, (int64_t)3}) {
    CHECK(fwo_decode(nullptr, &sc, b.data(), cut, FW_MEM_HOST, key.data(), nullptr, f1.data(), ts.data(), val.data(), 400,
                     wm.data(), wmp.data(), lm.data(), lmp.data(), 64, &cnt) == FW_OK);
    CHECK(cnt.consumed <= cut);
  }
  std::vector<uint8_t> bad = b;
  bad[4] = 9;   // a corrupt tag
  CHECK(fwo_decode(nullptr, &sc, bad.data(), (int64_t)bad.size(), FW_MEM_HOST, key.data(), nullptr, f1.data(), ts.data(),
                   val.data(), 400, wm.data(), wmp.data(), lm.data(), lmp.data(), 64, &cnt) == FW_ERR_INVALID_ARG);
  // too small a record capacity
  CHECK(fwo_decode(nullptr, &sc, b.data(), (int64_t)b.size(), FW_MEM_HOST, key.data(), nullptr, f1.data(), ts.data(),
                   val.data(), 10, wm.data(), wmp.data(), lm.data(), lmp.data(), 64, &cnt) == FW_ERR_CAPACITY);
}

static void kg_codec() {
  for (uint64_t round = 0; round < 200; ++round) {
    fwkg::BeOut o;
    std::vector<int64_t> xs;
    const int n = (int)(splitmix(round) % 64);
    for (int i = 0; i < n; ++i) {
      const int64_t x = (int64_t)splitmix(round * 977 + (uint64_t)i);
      xs.push_back(x);
      o.i64(x); o.i32((int32_t)x); o.i16((int32_t)(int16_t)x); o.u8((uint32_t)x & 0xff);
      double d; memcpy(&d, &x, 8); o.f64(d);
    }
    fwkg::BeIn in(o.b.data(), (int64_t)o.b.size());
    for (int i = 0; i < n; ++i) {
      CHECK(in.i64() == xs[(size_t)i]);
      CHECK(in.i32() == (int32_t)xs[(size_t)i]);
      CHECK(in.i16() == (int32_t)(int16_t)xs[(size_t)i]);
      CHECK(in.u8() == (int32_t)(xs[(size_t)i] & 0xff));
      (void)in.i64();
    }
    CHECK(in.done());
    (void)in.i64();            // past the end: flagged, nothing read
    CHECK(!in.ok);
    std::vector<size_t> idx((size_t)(splitmix(round + 5) % 300));
    for (size_t i = 0; i < idx.size(); ++i) idx[i] = i;
    fwkg::hashmap_order(idx, [&](size_t i) { return fwkg::timer_hash((int64_t)i * 1000 + 999, (int64_t)(i % 37), (int64_t)i * 1000,
                                                                     (int64_t)i * 1000 + 1000); },
                        [](size_t a, size_t b) { return a < b; });
    std::vector<char> seen(idx.size(), 0);
    for (size_t i : idx) { CHECK(i < seen.size() && !seen[i]); if (i < seen.size()) seen[i] = 1; }
  }
}

// a section cut to `len` bytes in a buffer of exactly that size, so that any read past it is an ASan report
static std::vector<uint8_t> cut(const std::vector<uint8_t>& b, size_t len) {
  return std::vector<uint8_t>(b.begin(), b.begin() + (ptrdiff_t)len);
}

// timer sections: set order, write / read round trips, cut and padded sections, the two corrupt counts
static void kg_timer_sections() {
  using fwkg::Timer;
  using fwkg::TimersFail;
  for (size_t n : {(size_t)0, (size_t)1, (size_t)2, (size_t)12, (size_t)13, (size_t)14, (size_t)30, (size_t)100}) {
    for (uint64_t round = 0; round < 4; ++round) {
      std::vector<Timer> t(n);
      for (size_t i = 0; i < n; ++i) {
        const int64_t start = (int64_t)(splitmix(round * 131 + i) % 50) * 1000 - 7000;
        t[i] = {(int64_t)i * 1000003 - 4000, start, start + 1000, start + 999 + (int64_t)(i % 2) * 250};   // (keys ascend)
      }
      // half of them restored, in reverse order: they lead their buckets in rank order
      std::map<Timer, int64_t> rank;
      if (round & 1) for (size_t i = 0; i < n; i += 2) rank[t[i]] = (int64_t)(n - i);
      const std::vector<Timer> ordered =
          fwkg::timers_in_set_order(n, [&](size_t i) { return t[i]; }, rank, [](size_t a, size_t b) { return a < b; });
      CHECK(ordered.size() == n);
      std::vector<Timer> a = t, b = ordered;
      std::sort(a.begin(), a.end());
      std::sort(b.begin(), b.end());
      CHECK(a == b);
      const uint32_t mask = fwkg::capacity_for(n) - 1;
      CHECK(n <= 12 ? mask == 15 : mask >= 31);   // more than 12 entries: the table doubled
      for (size_t i = 1; i < n; ++i) {
        const Timer &x = ordered[i - 1], &y = ordered[i];
        const uint32_t bx = (uint32_t)fwkg::spread(fwkg::timer_hash(x.ts, x.key, x.start, x.end)) & mask;
        const uint32_t by = (uint32_t)fwkg::spread(fwkg::timer_hash(y.ts, y.key, y.start, y.end)) & mask;
        CHECK(bx <= by);
        if (bx != by) continue;
        const bool rx = rank.count(x) != 0, ry = rank.count(y) != 0;
        CHECK(rx || !ry);                             // restored ones first
        if (rx && ry) CHECK(rank[x] < rank[y]);       // in blob order
        if (!rx && !ry) CHECK(x.key < y.key);         // then the caller's order (keys ascend with the index)
      }
      fwkg::BeOut o;
      fwkg::write_timers(o, ordered);
      CHECK(o.b.size() == 8 + 32 * n);
      std::vector<Timer> back;
      CHECK(fwkg::read_timers(o.b.data(), (int64_t)o.b.size(), back) == TimersFail::none);
      CHECK(back == ordered);
      for (size_t len = 0; len < o.b.size(); ++len) {
        const std::vector<uint8_t> c = cut(o.b, len);
        CHECK(fwkg::read_timers(c.data(), (int64_t)len, back) == TimersFail::truncated_or_trailing);
        CHECK(back.size() <= n);
      }
      std::vector<uint8_t> more = o.b;
      more.push_back(0);
      CHECK(fwkg::read_timers(more.data(), (int64_t)more.size(), back) == TimersFail::truncated_or_trailing);
      std::vector<uint8_t> neg = o.b;
      neg[0] = 0x80;
      CHECK(fwkg::read_timers(neg.data(), (int64_t)neg.size(), back) == TimersFail::negative_count);
      std::vector<uint8_t> proc = o.b;
      proc.back() = 1;
      CHECK(fwkg::read_timers(proc.data(), (int64_t)proc.size(), back) == TimersFail::processing_timers);
    }
  }
}

// "window-contents" tables: what a table's reader yields, written back in that (insertion) order, is the table
struct WcModel {
  struct Ent { int64_t start, end; fwkg::WcEntry e; };
  std::vector<Ent> ents;
};
static fwkg::WcFail wc_read(const std::vector<uint8_t>& b, const fwkg::WcLayout& L, WcModel& m) {
  m.ents.clear();
  fwkg::BeIn in(b.data(), (int64_t)b.size());
  const fwkg::WcFail f = fwkg::read_window_contents(
      in, L, [](int64_t, int64_t) { return true; },
      [&](int64_t s, int64_t e, fwkg::WcEntry& ent) { m.ents.push_back({s, e, ent}); return true; });
  return f == fwkg::WcFail::none && !in.done() ? fwkg::WcFail::truncated : f;
}
static std::vector<uint8_t> wc_write(const WcModel& m, const fwkg::WcLayout& L) {
  std::vector<fwkg::WcNamespace> ns =
      fwkg::group_namespaces(m.ents.size(), [&](size_t i) { return std::make_pair(m.ents[i].start, m.ents[i].end); });
  std::vector<size_t> first(ns.size());
  for (size_t w = 0; w < ns.size(); ++w) first[w] = ns[w].entries[0];
  fwkg::BeOut o;
  fwkg::write_window_contents(
      o, L, ns, [&](size_t a, size_t b) { return first[a] < first[b]; }, [&](size_t i) { return m.ents[i].e.key; },
      [](size_t a, size_t b) { return a < b; },
      [&](size_t i, fwkg::WcEntry& ent) { ent.word = m.ents[i].e.word; ent.el = m.ents[i].e.el; });
  return o.b;
}
static void kg_window_contents() {
  const int32_t reduce_fields[4] = {FW_SF_KEY, FW_SF_F1, FW_SF_SUM, FW_SF_MAX};
  const int32_t list_fields[3] = {FW_SF_KEY, FW_SF_VALUE, FW_SF_F1};
  const fwkg::WcLayout layouts[2] = {{reduce_fields, 4, false}, {list_fields, 3, true}};
  for (const fwkg::WcLayout& L : layouts) {
    for (uint64_t round = 0; round < 6; ++round) {
      // several namespaces sharing keys, entries in a scrambled insertion order
      WcModel m;
      const int n_ns = (int)(round % 4), n_keys = 1 + (int)(splitmix(round) % 20);
      for (int k = 0; k < n_keys; ++k)
        for (int w = 0; w < n_ns; ++w) {
          if (splitmix(round * 7 + (uint64_t)(k * 5 + w)) % 3 == 0) continue;
          WcModel::Ent x;
          x.start = (int64_t)w * 1000 - 1000;
          x.end = x.start + 1000;
          x.e.key = (int64_t)(splitmix((uint64_t)k + 99) >> (k % 2 ? 33 : 1)) - (k % 3 ? 0 : INT64_MAX / 2);
          if (L.list) {
            const int nel = 1 + (int)(splitmix((uint64_t)(k + w)) % 4);
            for (int q = 0; q < nel; ++q) x.e.el.push_back({(int64_t)splitmix(round + (uint64_t)q), (int64_t)(k * 10 + q)});
          } else {
            for (int f = 0; f < L.n_fields; ++f)
              x.e.word.push_back(L.field[f] == FW_SF_KEY ? x.e.key : (int64_t)splitmix(round * 13 + (uint64_t)(k * 4 + f)));
          }
          m.ents.insert(m.ents.begin() + (ptrdiff_t)(splitmix(round + m.ents.size()) % (m.ents.size() + 1)), x);
        }
      const std::vector<uint8_t> b = wc_write(m, L);
      WcModel back;
      CHECK(wc_read(b, L, back) == fwkg::WcFail::none);
      CHECK(back.ents.size() == m.ents.size());
      size_t found = 0;
      for (const auto& x : back.ents)
        for (const auto& y : m.ents)
          if (x.start == y.start && x.end == y.end && x.e.key == y.e.key) { CHECK(x.e.word == y.e.word && x.e.el == y.e.el); ++found; }
      CHECK(found == m.ents.size());
      CHECK(wc_write(back, L) == b);   // restored in blob order, the table is written back unchanged
      for (size_t len = 0; len < b.size(); ++len) CHECK(wc_read(cut(b, len), L, back) == fwkg::WcFail::truncated);
    }
  }
  // hand-built corrupt tables: one namespace [0, 1000), one entry of key 7
  auto table = [&](bool list, int32_t n_ns, int32_t n_ent, int32_t n_el, int64_t key_field) {
    fwkg::BeOut o;
    o.i32(n_ns); o.i64(0); o.i64(1000); o.i32(n_ent); o.i64(7);
    if (list) { o.i32(n_el); for (int q = 0; q < n_el; ++q) { o.i64(key_field); o.i64(40 + q); o.i64(50 + q); } }
    else { o.i64(key_field); o.i64(1); o.i64(2); o.i64(3); }
    return o.b;
  };
  WcModel back;
  CHECK(wc_read(table(false, 1, 1, 0, 7), layouts[0], back) == fwkg::WcFail::none && back.ents.size() == 1);
  CHECK(wc_read(table(false, 1, 1, 0, 8), layouts[0], back) == fwkg::WcFail::entry_key_differs);
  CHECK(wc_read(table(false, -1, 1, 0, 7), layouts[0], back) == fwkg::WcFail::negative_count);
  CHECK(wc_read(table(false, 1, -5, 0, 7), layouts[0], back) == fwkg::WcFail::negative_count);
  CHECK(wc_read(table(true, 1, 1, 2, 7), layouts[1], back) == fwkg::WcFail::none && back.ents.size() == 1 &&
        back.ents[0].e.el.size() == 2 && back.ents[0].e.el[1][0] == 41 && back.ents[0].e.el[1][1] == 51);
  CHECK(wc_read(table(true, 1, 1, 2, 8), layouts[1], back) == fwkg::WcFail::element_key_differs);
  CHECK(wc_read(table(true, 1, 1, 0, 7), layouts[1], back) == fwkg::WcFail::empty_list);
  CHECK(wc_read(table(true, 1, 1, -1, 7), layouts[1], back) == fwkg::WcFail::negative_list_size);
  // a callback that stops the read; the copy-out's size query, short buffers and an empty state section
  {
    const std::vector<uint8_t> b = table(false, 1, 1, 0, 7);
    fwkg::BeIn in(b.data(), (int64_t)b.size());
    CHECK(fwkg::read_window_contents(in, layouts[0], [](int64_t, int64_t) { return false; },
                                     [](int64_t, int64_t, fwkg::WcEntry&) { return true; }) == fwkg::WcFail::stopped);
    fwkg::BeOut st, tm, none;
    st.i64(1); st.u8(2);
    fwkg::write_timers(tm, {});
    int64_t ls = -1, lt = -1;
    CHECK(fwkg::copy_sections(st, tm, nullptr, 0, &ls, nullptr, 0, &lt) && ls == 9 && lt == 8);
    std::vector<uint8_t> bs(9), bt(8);
    CHECK(!fwkg::copy_sections(st, tm, bs.data(), 8, &ls, bt.data(), 8, &lt) && ls == 9);
    CHECK(!fwkg::copy_sections(st, tm, bs.data(), 9, &ls, bt.data(), 7, &lt));
    CHECK(!fwkg::copy_sections(st, tm, bs.data(), 9, &ls, nullptr, 0, &lt));
    CHECK(fwkg::copy_sections(st, tm, bs.data(), 9, &ls, bt.data(), 8, &lt) && bs == st.b && bt == tm.b);
    CHECK(fwkg::copy_sections(none, tm, bs.data(), 0, &ls, bt.data(), 8, &lt) && ls == 0);
  }
}

int main() {
  kg_codec();
  kg_timer_sections();
  kg_window_contents();
  decode_streams();
  // the window shapes
  struct Case { int assigner; int64_t size, slide, lateness; int trigger, agg, flags, vt, first; };
  const Case cases[] = {
      {FW_TUMBLING, 1000, 0, 0, FW_TRIGGER_EVENT_TIME, FW_AGG_SUM, 0, FW_VALUE_I64, 1},
      {FW_TUMBLING, 500, 0, 300, FW_TRIGGER_PURGING_EVENT_TIME, FW_AGG_SUM | FW_AGG_MAX, 0, FW_VALUE_I64, 1},
      {FW_TUMBLING, 1000, 0, 100, FW_TRIGGER_EVENT_TIME, FW_AGG_SUM | FW_AGG_COUNT, 0, FW_VALUE_I64, 1},
      {FW_SLIDING, 3000, 1000, 0, FW_TRIGGER_EVENT_TIME, FW_AGG_SUM | FW_AGG_MIN | FW_AGG_MAX | FW_AGG_COUNT, 0, FW_VALUE_F64, 1},
      {FW_SLIDING, 2500, 1000, 1200, FW_TRIGGER_EVENT_TIME, FW_AGG_SUM | FW_AGG_COUNT, 0, FW_VALUE_I64, 1},
      {FW_SESSION, 40, 0, 0, FW_TRIGGER_EVENT_TIME, FW_AGG_SUM | FW_AGG_COUNT, 0, FW_VALUE_I64, 0},
      {FW_SESSION, 40, 0, 500, FW_TRIGGER_PURGING_EVENT_TIME, FW_AGG_SUM, 0, FW_VALUE_F64, 0},
      {FW_TUMBLING, 1000, 0, 0, FW_TRIGGER_EVENT_TIME, FW_AGG_SUM, FW_AGGF_FOLD, FW_VALUE_I64, 0},
      {FW_TUMBLING, 1000, 0, 0, FW_TRIGGER_EVENT_TIME, FW_AGG_MAXBY, FW_AGGF_COMPARABLE, FW_VALUE_F64, 1},
      {FW_SLIDING, 2000, 1000, 0, FW_TRIGGER_EVENT_TIME, FW_AGG_LIST, 0, FW_VALUE_I64, 1},
  };
  for (const Case& k : cases) {
    fw_config c = base_config();
    c.assigner = k.assigner; c.size = k.size; c.slide = k.slide; c.allowed_lateness = k.lateness;
    c.trigger = k.trigger; c.agg_mask = k.agg; c.agg_flags = k.flags; c.value_type = k.vt; c.keep_first_f1 = k.first;
    if (k.flags & FW_AGGF_FOLD) c.fold_initial = 100;
    fw_engine* e = nullptr;
    const int rc = fwo_create(&c, &e);
    CHECK(rc == FW_OK);
    if (rc != FW_OK) { fprintf(stderr, "create: %s\n", fwo_last_error(nullptr)); continue; }
    const int64_t fired = drive(e, 40000, 300, -3000, k.lateness ? 900 : 0, k.vt == FW_VALUE_F64, k.lateness ? 200 : 1, 42);
    CHECK(fired > 0);
    fw_stats st;
    CHECK(fwo_get_stats(e, &st) == FW_OK);
    fwo_destroy(e);
  }
  // checkpoint layout: tumbling sum with first arrival, all int fields with the key
  {
    fw_config c = base_config();
    fw_state_layout L;
    memset(&L, 0, sizeof(L));
    L.n_fields = 3; L.field[0] = FW_SF_KEY; L.field[1] = FW_SF_F1; L.field[2] = FW_SF_SUM;
    snapshot_restore_roundtrip(c, 20000, L);
    c.agg_mask = FW_AGG_SUM | FW_AGG_MIN | FW_AGG_MAX | FW_AGG_COUNT;
    c.keep_first_f1 = 0;
    fw_state_layout M;
    memset(&M, 0, sizeof(M));
    M.n_fields = 5; M.field[0] = FW_SF_KEY; M.field[1] = FW_SF_SUM; M.field[2] = FW_SF_MIN; M.field[3] = FW_SF_MAX;
    M.field[4] = FW_SF_COUNT;
    snapshot_restore_roundtrip(c, 20000, M);
  }
  if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
  printf("host sanitize driver: ok\n");
  return 0;
}
