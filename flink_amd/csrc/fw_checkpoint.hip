// fw_checkpoint.hip — checkpoints of the engine's keyed state (included by fw_engine.hip): fw_snapshot_kg /
// fw_restore_kg (the engine's own blob) and fw_snapshot_kg_flink / fw_restore_kg_flink (the reference's key-group
// sections, for window and session state).  Host code, but for fw::k_sess_restore.  The reference layout's bytes —
// framing, HashMap order, truncation — are flink_kg_format.h's; this file maps panes to entries and timers and back
// (double min/max codes, fold, the windows an assigner allows, key groups, duplicates) and decides what a restore accepts.

// window panes hold state a checkpoint blob does not carry (the sliding assigner's extra windows)
static bool window_panes_used(fw_engine* e) {
  if (e->s.W == 0) return false;
  unsigned long long n = 0;
  if (hipMemcpy(&n, e->s.stats + ST_QUIRK, 8, hipMemcpyDeviceToHost) != hipSuccess) return true;
  return n > 0;
}

static void snap_header(const fw_engine* e, int32_t kg, int64_t n, int64_t* h) {
  const fw_config& c = e->cfg;
  const int64_t w[FW_SNAP_HEADER_WORDS] = {FW_SNAP_MAGIC, 2, kg, n, e->cur_wm, c.assigner, c.size,
                                          c.assigner == FW_SLIDING ? c.slide : c.size, c.offset, c.value_type,
                                          c.agg_mask, c.keep_first_f1 ? 1 : 0, c.allowed_lateness,
                                          (int64_t)c.trigger | ((int64_t)c.agg_flags << 8)};
  memcpy(h, w, sizeof(w));
}

// every key group's entries, from one copy of the directory and the live slices' columns.  The heap
// backend walks its per-key-group maps instead (HeapKeyedStateBackend.java:196-212); here the panes of
// all key groups sit in one dense table, so one pass sorts them into key groups
static int build_snapshot(fw_engine* e) {
  if (e->snap_epoch == e->state_epoch) return FW_OK;
  const fw::Spec& s = e->s;
  HIPCHK(e, hipStreamSynchronize(e->rstream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  int rc = check_device_error(e);
  if (rc) return rc;
  std::vector<int64_t> keys((size_t)s.D), tags((size_t)s.P);
  int32_t min_used = 0;
  HIPCHK(e, hipMemcpy(keys.data(), s.dir_keys, 8 * (size_t)s.D, hipMemcpyDeviceToHost));
  HIPCHK(e, hipMemcpy(tags.data(), s.slice_tag, 8 * (size_t)s.P, hipMemcpyDeviceToHost));
  HIPCHK(e, hipMemcpy(&min_used, s.dir_min_used, 4, hipMemcpyDeviceToHost));
  const int32_t mp = s.mp;
  std::vector<int32_t> kid_kg((size_t)s.stride, -1);
  for (int64_t k = 0; k < s.D; ++k)
    if (keys[k] != fw::EMPTY_KEY) kid_kg[k] = host_key_group(s, keys[k]);
  if (min_used) kid_kg[s.D] = host_key_group(s, fw::EMPTY_KEY);
  e->snap_kg.assign((size_t)mp, {});
  e->snap_wkg.assign((size_t)mp, {});
  e->snap_unarmed.clear();
  e->snap_has_key.assign((size_t)mp, 0);
  e->snap_any_key = false;
  for (size_t k = 0; k < kid_kg.size(); ++k)
    if (kid_kg[k] >= 0) { e->snap_has_key[(size_t)kid_kg[k]] = 1; e->snap_any_key = true; }
  if (e->kg_evicted) {   // key groups whose keys were all evicted still had state (StateTable.get(kg) != null)
    std::vector<uint8_t> ev((size_t)mp);
    HIPCHK(e, hipMemcpy(ev.data(), e->kg_evicted, (size_t)mp, hipMemcpyDeviceToHost));
    for (int32_t k = 0; k < mp; ++k) if (ev[(size_t)k]) { e->snap_has_key[(size_t)k] = 1; e->snap_any_key = true; }
  }
  if (e->list) {   // list state (tumbling): the slices' element buffers, grouped by (window, key) in arrival order
    e->snap_list.clear();
    std::vector<unsigned long long> lc((size_t)s.P);
    HIPCHK(e, hipMemcpy(lc.data(), e->lst.cnt, 8 * (size_t)s.P, hipMemcpyDeviceToHost));
    std::vector<int64_t> rows;
    for (int32_t p = 0; p < s.P; ++p) {
      const int64_t m = tags[(size_t)p];
      if (m == fw::FREE_TAG) continue;
      const int64_t ne = std::min<int64_t>((int64_t)lc[(size_t)p], e->lst.cap);
      rows.resize((size_t)ne * LST_WORDS);
      if (ne > 0)
        HIPCHK(e, hipMemcpy(rows.data(), e->lst.buf + (size_t)p * (size_t)e->lst.cap * LST_WORDS, 8 * rows.size(),
                            hipMemcpyDeviceToHost));
      std::vector<uint8_t> armed;
      if (e->disarmed.count(m)) {   // a restored window that fired before: the keys no record re-armed since
        armed.resize((size_t)s.stride);
        HIPCHK(e, hipMemcpy(armed.data(), s.armed + (size_t)p * (size_t)s.stride, (size_t)s.stride, hipMemcpyDeviceToHost));
      }
      for (int64_t j = 0; j < ne; ++j) {
        const int64_t* x = &rows[(size_t)j * LST_WORDS];   // kid, ordinal, value, f1
        if (x[0] < 0 || x[0] >= s.stride || kid_kg[(size_t)x[0]] < 0) continue;
        const int64_t key = x[0] == s.D ? fw::EMPTY_KEY : keys[(size_t)x[0]];
        e->snap_list[{m, key}].push_back({x[1], x[2], x[3]});
        if (!armed.empty() && !armed[(size_t)x[0]]) e->snap_unarmed.insert({m, key});
      }
    }
    for (auto& kv : e->snap_list) {
      std::sort(kv.second.begin(), kv.second.end());
      const int64_t key = kv.first.second;
      const int64_t ent[FW_SNAP_ENTRY_WORDS] = {kv.first.first, key, 0, INT64_MAX, INT64_MIN, 0,
                                                kv.second[0][0] - e->ordinal, 0};
      auto& v = e->snap_kg[(size_t)host_key_group(s, key)];
      v.insert(v.end(), ent, ent + FW_SNAP_ENTRY_WORDS);
    }
    e->snap_gkg.assign((size_t)mp, {});
    e->snap_epoch = e->state_epoch;
    return FW_OK;
  }
  const size_t st = (size_t)s.stride;
  std::vector<int64_t> sum(st), mn, mx, cnt, first, f1v;
  std::vector<uint8_t> present;
  // one slot's columns (a slice's, or a sliding window's own pane) as entries under `tag`.  `dis`: a restored
  // window that fired before — its panes no record re-armed since are unarmed (a window pane: every such key)
  auto slot_entries = [&](const fw::Cols& col, size_t slot, int64_t tag, bool dis, bool all_keys,
                          std::vector<std::vector<int64_t>>& dest) -> int {
    const size_t off = slot * st;
    auto get = [&](std::vector<int64_t>& v, const int64_t* c) -> hipError_t {
      if (!c) return hipSuccess;
      v.resize(st);
      return hipMemcpy(v.data(), c + off, 8 * st, hipMemcpyDeviceToHost);
    };
    HIPCHK(e, get(sum, col.sum));
    HIPCHK(e, get(mn, col.mn));
    HIPCHK(e, get(mx, col.mx));
    HIPCHK(e, get(cnt, col.cnt));
    if (s.first) {
      HIPCHK(e, get(first, col.first));
      HIPCHK(e, get(f1v, col.f1v));
    } else {
      present.resize(st);
      HIPCHK(e, hipMemcpy(present.data(), col.present + off, st, hipMemcpyDeviceToHost));
    }
    std::vector<uint8_t> armed;
    if (dis) {
      armed.resize(st);
      HIPCHK(e, hipMemcpy(armed.data(), s.armed + off, st, hipMemcpyDeviceToHost));
    }
    for (size_t k = 0; k < st; ++k) {
      if (kid_kg[k] < 0) continue;
      const bool pres = s.first ? first[k] != INT64_MAX : present[k] != 0;
      const int64_t key = (int64_t)k == s.D ? fw::EMPTY_KEY : keys[k];
      if (dis && !armed[k] && (pres || all_keys)) e->snap_unarmed.insert({tag, key});
      if (!pres) continue;
      const int64_t ent[FW_SNAP_ENTRY_WORDS] = {
          tag, key, sum[k], col.mn ? mn[k] : INT64_MAX, col.mx ? mx[k] : INT64_MIN,
          col.cnt ? (s.by ? cnt[k] - e->ordinal : cnt[k]) : 0,
          s.first ? first[k] - e->ordinal : -1, s.first ? f1v[k] : 0};
      auto& v = dest[(size_t)kid_kg[k]];
      v.insert(v.end(), ent, ent + FW_SNAP_ENTRY_WORDS);
    }
    return FW_OK;
  };
  for (int32_t p = 0; p < s.P; ++p)
    if (tags[p] != fw::FREE_TAG)
      if (int rc = slot_entries(s.c, (size_t)p, tags[p], s.assigner != FW_SLIDING && e->disarmed.count(tags[p]) != 0, false, e->snap_kg))
        return rc;
  // sliding: the windows' own panes (restored window state, records below offset - slide)
  if (s.W > 0) {
    std::vector<int64_t> wtags((size_t)s.W);
    HIPCHK(e, hipMemcpy(wtags.data(), s.wtag, 8 * (size_t)s.W, hipMemcpyDeviceToHost));
    for (int32_t w = 0; w < s.W; ++w)
      if (wtags[(size_t)w] != fw::FREE_TAG)
        if (int rc = slot_entries(s.wc, (size_t)w, wtags[(size_t)w], e->disarmed.count(wtags[(size_t)w]) != 0, true, e->snap_wkg))
          return rc;
  }
  // purged windows' cleanup timers (PurgingTrigger + allowed lateness)
  e->snap_gkg.assign((size_t)mp, {});
  for (int64_t m : e->ghost_windows) {
    const size_t off = (size_t)floor_mod(m, s.P) * st;
    std::vector<int64_t> g(st);
    HIPCHK(e, hipMemcpy(g.data(), s.gfirst + off, 8 * st, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < st; ++k) {
      if (g[k] == INT64_MAX || kid_kg[k] < 0) continue;
      const int64_t key = (int64_t)k == s.D ? fw::EMPTY_KEY : keys[k];
      auto& v = e->snap_gkg[(size_t)kid_kg[k]];
      v.insert(v.end(), {m, key, s.first ? g[k] - e->ordinal : -1});
    }
  }
  e->snap_epoch = e->state_epoch;
  return FW_OK;
}

extern "C" int fw_snapshot_kg(fw_engine* e, int32_t kg, void* buf, int64_t cap, int64_t* len) {
  if (!e || !len) return FW_ERR_INVALID_ARG;
  if (e->session) return reject(e, FW_ERR_UNSUPPORTED, "session windows: the merging-window set is keyed list state of its own (no checkpoint)");
  if (e->list) return reject(e, FW_ERR_UNSUPPORTED, "list state: buffered elements have no checkpoint layout here");
  if (window_panes_used(e)) return reject(e, FW_ERR_UNSUPPORTED, "sliding windows: records below offset - slide put state in window panes, which no checkpoint layout carries");
  if (!e->disarmed.empty())
    return reject(e, FW_ERR_UNSUPPORTED, "restored windows without trigger timers: only the reference layout (explicit "
                                         "timers, fw_snapshot_kg_flink) carries them");
  if (e->s.gtag && !e->ghost_windows.empty())
    return reject(e, FW_ERR_UNSUPPORTED, "PurgingTrigger with allowed lateness: purged windows within their lateness keep "
                                         "cleanup timers without state, which only the reference layout "
                                         "(fw_snapshot_kg_flink) carries");
  if (e->sticky) return e->sticky;
  if (kg < e->s.kg_start || kg > e->s.kg_end)   // HeapInternalTimerService.restoreTimersForKeyGroup's check
    return reject(e, FW_ERR_INVALID_ARG, "Key Group " + std::to_string(kg) + " does not belong to the local range.");
  if (e->used_key_hash)
    return reject(e, FW_ERR_UNSUPPORTED, "snapshot needs Long keys (a push carried Java key hashes)");
  HIPCHK(e, hipSetDevice(e->dev));
  int rc = build_snapshot(e);
  if (rc) return rc;
  const std::vector<int64_t>& v = e->snap_kg[(size_t)kg];
  const int64_t n = (int64_t)v.size() / FW_SNAP_ENTRY_WORDS;
  *len = 8 * (FW_SNAP_HEADER_WORDS + (int64_t)v.size());
  if (!buf) return FW_OK;
  if (cap < *len) return reject(e, FW_ERR_CAPACITY, "snapshot buffer too small");
  snap_header(e, kg, n, (int64_t*)buf);
  if (!v.empty()) memcpy((int64_t*)buf + FW_SNAP_HEADER_WORDS, v.data(), 8 * v.size());
  return FW_OK;
}

// restored rows to the device, launch(rows on the device) on the engine's stream, and the outcome once it ran
template <class Launch>
static int launch_on_rows(fw_engine* e, const int64_t* rows, size_t words, Launch launch) {
  int64_t* d = nullptr;
  HIPCHK(e, hipMalloc(&d, 8 * words));
  hipError_t r = hipMemcpyAsync(d, rows, 8 * words, hipMemcpyHostToDevice, e->stream);
  if (r == hipSuccess) {
    launch(d);
    r = hipGetLastError();
  }
  const hipError_t r2 = hipStreamSynchronize(e->stream);
  (void)hipFree(d);
  HIPCHK(e, r);
  HIPCHK(e, r2);
  return check_device_error(e);
}

// load n validated snapshot entries (FW_SNAP_ENTRY_WORDS each) and set the watermark
static int restore_entries(fw_engine* e, int64_t wm, const int64_t* ent, int64_t n, int32_t wpane = 0) {
  HIPCHK(e, hipSetDevice(e->dev));
  e->restored = true;
  e->cur_wm = wm;
  e->state_epoch++;
  if (n == 0) return FW_OK;
  return launch_on_rows(e, ent, (size_t)n * FW_SNAP_ENTRY_WORDS, [&](int64_t* d) {
    const int blocks = (int)std::min<int64_t>((n + BLOCK - 1) / BLOCK, 1024);
    hipLaunchKernelGGL(fw::k_restore, dim3(blocks), dim3(BLOCK), 0, e->stream, e->s, d, n, wpane);
  });
}

extern "C" int fw_restore_kg(fw_engine* e, int32_t kg, const void* buf, int64_t len) {
  if (!e || !buf) return FW_ERR_INVALID_ARG;
  if (e->session) return reject(e, FW_ERR_UNSUPPORTED, "session windows: the merging-window set is keyed list state of its own (no checkpoint)");
  if (e->list) return reject(e, FW_ERR_UNSUPPORTED, "list state: buffered elements have no checkpoint layout here");
  if (e->sticky) return e->sticky;
  if (e->pushes > 0 || e->records_in > 0) return reject(e, FW_ERR_INVALID_ARG, "restore after the first push");
  if (len < 8 * FW_SNAP_HEADER_WORDS) return reject(e, FW_ERR_INVALID_ARG, "snapshot blob too short");
  const int64_t* h = (const int64_t*)buf;
  int64_t ref[FW_SNAP_HEADER_WORDS];
  snap_header(e, kg, h[3], ref);
  if (h[0] != FW_SNAP_MAGIC || h[1] != 2) return reject(e, FW_ERR_INVALID_ARG, "not a key-group snapshot (magic/version)");
  if (h[2] != kg) return reject(e, FW_ERR_INVALID_ARG, "snapshot holds key group " + std::to_string(h[2]));
  for (int w = 5; w < FW_SNAP_HEADER_WORDS; ++w)
    if (h[w] != ref[w]) return reject(e, FW_ERR_INVALID_ARG, "snapshot of a different window/reduce configuration");
  if (kg < e->s.kg_start || kg > e->s.kg_end)
    return reject(e, FW_ERR_INVALID_ARG, "Key Group " + std::to_string(kg) + " does not belong to the local range.");
  const int64_t n = h[3];
  if (n < 0 || len != 8 * (FW_SNAP_HEADER_WORDS + n * FW_SNAP_ENTRY_WORDS))
    return reject(e, FW_ERR_INVALID_ARG, "snapshot blob length does not match its entry count");
  if (e->restored && h[4] != e->cur_wm)
    return reject(e, FW_ERR_INVALID_ARG, "key groups checkpointed at different watermarks");
  const int64_t* ent = h + FW_SNAP_HEADER_WORDS;
  for (int64_t j = 0; j < n; ++j)
    if (host_key_group(e->s, ent[j * FW_SNAP_ENTRY_WORDS + 1]) != kg)
      return reject(e, FW_ERR_KEY_GROUP, "snapshot entry key outside its key group");
  if (int rc = restore_entries(e, h[4], ent, n)) return rc;
  // PurgingTrigger + allowed lateness: the windows within their lateness at the restored watermark are tracked
  // for their cleanup timers as after any watermark (fw_snapshot_kg took none with such timers pending)
  if (e->s.gtag) return ghost_advance(e, INT64_MIN, e->cur_wm);
  return FW_OK;
}

// ------------------------------------------------------------------------------------------------
// checkpoint state in the reference's key-group layout (flink_kg_format.h; flink_window.h)
// ------------------------------------------------------------------------------------------------

// one (window, key) entry of a key group's state table, engine encodings (double bits, min/max codes)
struct KgPane {
  int64_t start, end, key;
  int64_t sum, mn, mx, cnt;
  int64_t first;    // first-arrival ordinal (0 when the config does not track first arrival)
  int64_t f1;
  bool unarmed;     // a restored window's pane whose trigger timer fired before the checkpoint (none pending)
  int64_t m = 0;    // tumbling: the slice (= window) number
};

static int check_state_layout(fw_engine* e, const fw_state_layout* L) {
  if (!L || L->n_fields < 0 || L->n_fields > FW_SF_MAX_FIELDS)
    return reject(e, FW_ERR_INVALID_ARG, "bad state layout");
  int seen[FW_SF_VALUE + 1] = {0};
  for (int i = 0; i < L->n_fields; ++i) {
    const int f = L->field[i];
    if (f < FW_SF_KEY || f > FW_SF_VALUE) return reject(e, FW_ERR_INVALID_ARG, "bad state layout field");
    seen[f]++;
  }
  const fw_config& c = e->cfg;
  const bool by = e->s.by;
  if (e->list) {   // ListSerializer's element: the window's input tuple — its key, f1 and value fields, in order
    if (seen[FW_SF_KEY] > 1 || seen[FW_SF_F1] > 1 || seen[FW_SF_VALUE] != 1 || seen[FW_SF_SUM] || seen[FW_SF_MIN] ||
        seen[FW_SF_MAX] || seen[FW_SF_COUNT])
      return reject(e, FW_ERR_INVALID_ARG, "list state layout: the element tuple's fields, FW_SF_VALUE once and "
                                           "FW_SF_KEY / FW_SF_F1 at most once");
    return FW_OK;
  }
  const int want[FW_SF_VALUE + 1] = {0, -1, c.keep_first_f1 || by ? 1 : 0, !by && (c.agg_mask & FW_AGG_SUM) ? 1 : 0,
                                     !by && (c.agg_mask & FW_AGG_MIN) ? 1 : 0, !by && (c.agg_mask & FW_AGG_MAX) ? 1 : 0,
                                     !by && (c.agg_mask & FW_AGG_COUNT) ? 1 : 0, by ? 1 : 0};
  if (seen[FW_SF_KEY] > 1) return reject(e, FW_ERR_INVALID_ARG, "state layout names the key twice");
  for (int f = FW_SF_F1; f <= FW_SF_VALUE; ++f)
    if (seen[f] != want[f])
      return reject(e, FW_ERR_INVALID_ARG, "state layout must name each computed aggregate (and f1 iff "
                                           "keep_first_f1) exactly once");
  return FW_OK;
}

// HeapFoldingState holds the accumulator: the fold's initial value folded with the pane (as emit_record
// applies it), and back (sum and count subtract it: exact for Long, to the last bit for doubles only when
// the initial value is 0; min and max hold it already: the accumulator is at or beyond it)
static KgPane fold_pane(const fw_engine* e, KgPane p) {
  const fw::Spec& s = e->s;
  const int64_t x = s.fold_init;
  if (s.vt == FW_VALUE_I64) p.sum = fw::jadd(x, p.sum);
  else { double a, b; memcpy(&a, &x, 8); memcpy(&b, &p.sum, 8); b = a + b; memcpy(&p.sum, &b, 8); }
  p.mn = std::min(p.mn, fw::min_code(s.vt, s.cmpto, x));
  p.mx = std::max(p.mx, fw::max_code(s.vt, s.cmpto, x));
  p.cnt = fw::jadd(x, p.cnt);
  return p;
}
static KgPane unfold_pane(const fw_engine* e, KgPane p) {
  const fw::Spec& s = e->s;
  const int64_t x = s.fold_init;
  if (s.vt == FW_VALUE_I64) p.sum = fw::jsub(p.sum, x);
  else { double a, b; memcpy(&a, &x, 8); memcpy(&b, &p.sum, 8); b = b - a; memcpy(&p.sum, &b, 8); }
  p.cnt = fw::jsub(p.cnt, x);
  return p;
}

// a value held as bits (a double's, for FW_VALUE_F64) as the word its Java type serializes to
static int64_t value_word(const fw_engine* e, int64_t bits) {
  return e->s.vt == FW_VALUE_F64 ? fwkg::double_word(bits) : bits;
}

// the pane's value words, one per layout field
static void pane_words(const fw_engine* e, const fw_state_layout* L, const KgPane& p_in, std::vector<int64_t>& word) {
  const KgPane p = e->s.fold ? fold_pane(e, p_in) : p_in;
  auto code = [&](int64_t c) {
    if (e->s.vt != FW_VALUE_F64) return c;
    const double d = fw::f64_from_code(c);
    int64_t bits;
    memcpy(&bits, &d, 8);
    return fwkg::double_word(bits);
  };
  for (int f = 0; f < L->n_fields; ++f) {
    int64_t w = 0;
    switch (L->field[f]) {
      case FW_SF_KEY: w = p.key; break;
      case FW_SF_F1: w = p.f1; break;
      case FW_SF_SUM: w = value_word(e, p.sum); break;
      case FW_SF_MIN: w = code(p.mn); break;
      case FW_SF_MAX: w = code(p.mx); break;
      case FW_SF_COUNT: w = p.cnt; break;
      case FW_SF_VALUE: w = code(e->cfg.agg_mask == FW_AGG_MAXBY ? p.mx : p.mn); break;
    }
    word.push_back(w);
  }
}

// and back: a restored entry's words into the pane, in the engine's encodings (not yet unfolded)
static void pane_from_words(const fw_engine* e, const fw_state_layout* L, const std::vector<int64_t>& word, KgPane& p) {
  const bool f64 = e->s.vt == FW_VALUE_F64, cmpto = e->s.cmpto;
  for (size_t f = 0; f < word.size(); ++f) {   // (list state: no words)
    const int64_t x = word[f];
    double d;
    memcpy(&d, &x, 8);
    switch (L->field[f]) {
      case FW_SF_KEY: break;   // (equal to the entry's key: read_window_contents)
      case FW_SF_F1: p.f1 = x; break;
      case FW_SF_SUM: p.sum = x; break;
      case FW_SF_MIN: p.mn = f64 ? (cmpto ? fw::f64_cmp_code(d) : fw::f64_min_code(d)) : x; break;
      case FW_SF_MAX: p.mx = f64 ? (cmpto ? fw::f64_cmp_code(d) : fw::f64_max_code(d)) : x; break;
      case FW_SF_COUNT: p.cnt = x; break;
      case FW_SF_VALUE: p.mn = p.mx = f64 ? fw::f64_cmp_code(d) : x; break;
    }
  }
}

static fwkg::WcLayout wc_layout(const fw_engine* e, const fw_state_layout* L) { return {L->field, L->n_fields, e->list}; }

// a read_window_contents / read_timers failure as the restore's rejection
static int reject_state(fw_engine* e, fwkg::WcFail f) {
  switch (f) {
    case fwkg::WcFail::negative_count: return reject(e, FW_ERR_INVALID_ARG, "corrupt state section");
    case fwkg::WcFail::negative_list_size: return reject(e, FW_ERR_INVALID_ARG, "corrupt list state");
    case fwkg::WcFail::empty_list: return reject(e, FW_ERR_INVALID_ARG, "empty list state entry");
    case fwkg::WcFail::entry_key_differs: return reject(e, FW_ERR_UNSUPPORTED, "state key field differs from the key");
    case fwkg::WcFail::element_key_differs: return reject(e, FW_ERR_UNSUPPORTED, "element key field differs from the key");
    default: return reject(e, FW_ERR_INVALID_ARG, "state section truncated or with trailing bytes");
  }
}
static int read_timer_section(fw_engine* e, const void* timers, int64_t timers_len, std::vector<fwkg::Timer>& got) {
  switch (fwkg::read_timers(timers, timers_len, got)) {
    case fwkg::TimersFail::none: return FW_OK;
    case fwkg::TimersFail::negative_count: return reject(e, FW_ERR_INVALID_ARG, "corrupt timer section");
    case fwkg::TimersFail::processing_timers: return reject(e, FW_ERR_UNSUPPORTED, "processing-time timers");
    default: return reject(e, FW_ERR_INVALID_ARG, "timer section truncated or with trailing bytes");
  }
}

// the last steps of both snapshot bodies: the timers in the JVM's set order, then both sections out
template <class At, class Earlier>
static int finish_sections(fw_engine* e, fwkg::BeOut& st, size_t n_timers, At at, Earlier earlier, void* state,
                           int64_t state_cap, int64_t* state_len, void* timers, int64_t timers_cap, int64_t* timers_len) {
  fwkg::BeOut tm;
  fwkg::write_timers(tm, fwkg::timers_in_set_order(n_timers, at, e->restored_timer_rank, earlier));
  if (!fwkg::copy_sections(st, tm, state, state_cap, state_len, timers, timers_cap, timers_len))
    return reject(e, FW_ERR_CAPACITY, "snapshot buffer too small");
  return FW_OK;
}

// The panes of key group kg as the reference holds them: one per (window, key).  Tumbling: a slice is a
// window.  Sliding: every window still in its lifetime (cleanup time > watermark) that a slice of the key
// overlaps, combined from its slices in slice order (double sums: the slice-sum order, not arrival order)
static void kg_panes(const fw_engine* e, int32_t kg, std::vector<KgPane>& out) {
  const fw_config& c = e->cfg;
  const fw::Spec& s = e->s;
  const std::vector<int64_t>& v = e->snap_kg[(size_t)kg];
  const size_t n = v.size() / FW_SNAP_ENTRY_WORDS;
  const bool tumbling = c.assigner == FW_TUMBLING;
  auto pane_of = [&](const int64_t* x, int64_t start) {
    KgPane p;
    p.start = start;
    p.end = fw::jadd(start, c.size);
    p.key = x[1];
    p.sum = x[2]; p.mn = x[3]; p.mx = x[4];
    p.cnt = x[5];               // maxBy/minBy: the extremal record's ordinal
    p.first = s.first ? x[6] : 0;
    p.f1 = x[7];
    p.unarmed = e->snap_unarmed.count({x[0], x[1]}) != 0 && tumbling;
    p.m = x[0];
    return p;
  };
  out.clear();
  if (tumbling) {
    for (size_t j = 0; j < n; ++j) {
      const int64_t* x = &v[j * FW_SNAP_ENTRY_WORDS];
      KgPane p = pane_of(x, host_window_start(c, x[0]));
      if (fw::cleanup_time(fw::jsub(p.end, 1), c.allowed_lateness) > e->cur_wm) out.push_back(p);
    }
    return;
  }
  std::vector<size_t> ord(n);
  for (size_t j = 0; j < n; ++j) ord[j] = j;
  std::sort(ord.begin(), ord.end(), [&](size_t a, size_t b) {
    const int64_t* x = &v[a * FW_SNAP_ENTRY_WORDS];
    const int64_t* y = &v[b * FW_SNAP_ENTRY_WORDS];
    return x[1] != y[1] ? x[1] < y[1] : x[0] < y[0];
  });
  std::map<std::pair<int64_t, int64_t>, KgPane> win;   // (window number, key)
  const bool f64 = s.vt == FW_VALUE_F64;
  // the windows' own panes first (restored window state: the earlier arrivals), then each slice into every
  // window it makes up
  const std::vector<int64_t>& wv = e->snap_wkg[(size_t)kg];
  std::vector<std::pair<int64_t, const int64_t*>> items;   // (window number or -1 for a slice, entry)
  for (size_t j = 0; j < wv.size() / FW_SNAP_ENTRY_WORDS; ++j) items.push_back({1, &wv[j * FW_SNAP_ENTRY_WORDS]});
  for (size_t j : ord) items.push_back({0, &v[j * FW_SNAP_ENTRY_WORDS]});
  for (const auto& item : items) {
    const int64_t* x = item.second;
    const int64_t m = x[0];
    const int64_t w_lo = item.first ? m : fw::floor_div(m - s.K, s.R) + 1, w_hi = item.first ? m : fw::floor_div(m, s.R);
    for (int64_t w = w_lo; w <= w_hi; ++w) {
      const int64_t start = host_window_start(c, w);
      if (fw::cleanup_time(fw::jsub(fw::jadd(start, c.size), 1), c.allowed_lateness) <= e->cur_wm) continue;
      KgPane b = pane_of(x, start);
      auto it = win.find({w, b.key});
      if (it == win.end()) { win.emplace(std::make_pair(w, b.key), b); continue; }
      KgPane& a = it->second;
      if (s.by) {   // the extremal record; a tie keeps the earlier one (maxBy/minBy(first = false): the later)
        const bool maxby = c.agg_mask == FW_AGG_MAXBY;
        const int64_t ca = maxby ? a.mx : a.mn, cb = maxby ? b.mx : b.mn;
        const bool better = maxby ? cb > ca : cb < ca;
        const bool tie_later = (c.agg_flags & FW_AGGF_BY_LAST) != 0;
        if (better || (cb == ca && (tie_later ? b.cnt > a.cnt : b.cnt < a.cnt))) {
          a.mx = b.mx; a.mn = b.mn; a.cnt = b.cnt; a.f1 = b.f1;
        }
        a.first = std::min(a.first, b.first);
        continue;
      }
      if (f64) {
        double da, db;
        memcpy(&da, &a.sum, 8); memcpy(&db, &b.sum, 8);
        da += db;
        memcpy(&a.sum, &da, 8);
      } else {
        a.sum = fw::jadd(a.sum, b.sum);
      }
      a.mn = std::min(a.mn, b.mn);
      a.mx = std::max(a.mx, b.mx);
      a.cnt = fw::jadd(a.cnt, b.cnt);
      if (s.first && b.first < a.first) { a.first = b.first; a.f1 = b.f1; }
    }
  }
  for (auto& kv : win) {   // (sliding: a window restored disarmed and not re-armed for the key)
    kv.second.unarmed = e->snap_unarmed.count({kv.first.first, kv.first.second}) != 0;
    if (!e->list_entry_rank.empty()) {   // a restored list entry keeps its place in the namespace's insertion order
      auto it = e->list_entry_rank.find({kv.second.start, kv.second.key});
      if (it != e->list_entry_rank.end()) kv.second.first = it->second - e->ordinal;
    }
    out.push_back(kv.second);
  }
}

// ------------------------------------------------------------------------------------------------
// session windows in the reference's key-group layout: WindowOperator keeps two keyed states for a merging
// assigner (WindowOperator.java:445-460, 724-736) — "window-contents" (the reducing state, namespace = each
// in-flight window's STATE window) and "merging-window-set" (ListState<Tuple2<W, W>> in VoidNamespace: per
// key its in-flight windows and their state windows, MergingWindowSet.persist, MergingWindowSet.java:91-95).
// stateTables iterates "window-contents" (HashMap bucket 12 of 16) before "merging-window-set" (bucket 15): ids
// 0 and 1.  Engine side: k_sess_walk / k_sess_walk_hot / k_sess_wm keep per slot the state window and the
// arrival ordinals that place each entry in its HashMap's insertion order (SessDev).
// ------------------------------------------------------------------------------------------------
namespace fw {
// restored sessions: one row per in-flight window (key, slot, start, end, state-window start, its entry's rank,
// trigger pending, sum, min / max codes, count, f1); key ids by the directory's insert
constexpr int SESS_ROW = 15;
__global__ __launch_bounds__(BLOCK) void k_sess_restore(Spec s, SessDev d, const int64_t* rows, int64_t n, int64_t put0) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t* r = rows + i * SESS_ROW;
  const int64_t kid = dir_find_or_insert(s, r[0]);
  if (kid < 0) { cap_error(s, 20); return; }
  const int q = (int)r[1];
  const int64_t x = kid * d.sw + q;
  d.start[x] = r[2];
  d.end[x] = r[3];
  d.sws[x] = r[4];
  d.swc[x] = r[5];
  d.put[x] = put0 + q;             // MergingWindowSet(assigner, state): puts in list order
  d.cre[x] = d.tre[x] = put0;      // (restored timers are ordered by their blob rank)
  if (d.sum) d.sum[x] = r[7];
  if (d.mn) d.mn[x] = r[8];
  if (d.mx) d.mx[x] = r[9];
  if (d.cnt) d.cnt[x] = r[10];
  if (d.f1) d.f1[x] = r[11];
  if (d.list) {   // list state: the window's elements, chained in pool entries the host laid out
    d.head[x] = r[12];
    d.tail[x] = r[13];
    d.len[x] = r[14];
  }
  sess_ns_add(d, record_key_group(s, long_hash_code(r[0])), r[4]);
  atomicOr(&d.live[kid * d.nw + (q >> 6)], 1ull << (q & 63));
  if (r[6]) atomicOr(&d.trig[kid * d.nw + (q >> 6)], 1ull << (q & 63));
}
}  // namespace fw

static int session_download(fw_engine* e) {
  fw_engine::SessHost& h = e->sess_host;
  if (h.epoch == e->state_epoch && h.wm == e->cur_wm) return FW_OK;
  const fw::Spec& s = e->s;
  const SessDev& d = e->sess;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if (int rc = check_device_error(e)) return rc;
  const size_t cells = (size_t)d.sw * (size_t)s.stride, rows = (size_t)s.stride;
  auto get = [&](std::vector<int64_t>& v, const int64_t* p, size_t n) -> hipError_t {
    v.assign(p ? n : 0, 0);
    return p ? hipMemcpy(v.data(), p, 8 * n, hipMemcpyDeviceToHost) : hipSuccess;
  };
  HIPCHK(e, get(h.keys, s.dir_keys, (size_t)s.D));
  HIPCHK(e, get(h.st, d.start, cells));
  HIPCHK(e, get(h.en, d.end, cells));
  HIPCHK(e, get(h.sws, d.sws, cells));
  HIPCHK(e, get(h.swc, d.swc, cells));
  HIPCHK(e, get(h.put, d.put, cells));
  HIPCHK(e, get(h.cre, d.cre, cells));
  HIPCHK(e, get(h.tre, d.tre, cells));
  HIPCHK(e, get(h.sum, d.sum, cells));
  HIPCHK(e, get(h.mn, d.mn, cells));
  HIPCHK(e, get(h.mx, d.mx, cells));
  HIPCHK(e, get(h.cnt, d.cnt, cells));
  HIPCHK(e, get(h.f1, d.f1, cells));
  HIPCHK(e, get(h.ktouch, d.ktouch, rows));
  HIPCHK(e, get(h.lhead, d.list ? d.head : nullptr, cells));
  HIPCHK(e, get(h.llen, d.list ? d.len : nullptr, cells));
  HIPCHK(e, get(h.pv, d.list ? d.pv : nullptr, (size_t)d.pcap));
  HIPCHK(e, get(h.pf1, d.list ? d.pf1 : nullptr, (size_t)d.pcap));
  HIPCHK(e, get(h.pnext, d.list ? d.pnext : nullptr, (size_t)d.pcap));
  HIPCHK(e, get(h.ktts, d.ktts, rows));
  h.kacc.assign(rows, 0);
  HIPCHK(e, hipMemcpy(h.kacc.data(), d.kacc, 4 * rows, hipMemcpyDeviceToHost));
  unsigned long long nl = 0;
  HIPCHK(e, hipMemcpy(&nl, d.nslog_n, 8, hipMemcpyDeviceToHost));
  if (int rc = session_ns_lost(e, &h.nslog_over)) return rc;   // a live namespace lacks a dropped entry
  HIPCHK(e, get(h.nslog, d.nslog, 4 * (size_t)std::min<int64_t>((int64_t)nl, d.nslog_cap)));
  h.live.assign(rows * (size_t)d.nw, 0);
  h.trig.assign(rows * (size_t)d.nw, 0);
  HIPCHK(e, hipMemcpy(h.live.data(), d.live, 8 * h.live.size(), hipMemcpyDeviceToHost));
  HIPCHK(e, hipMemcpy(h.trig.data(), d.trig, 8 * h.trig.size(), hipMemcpyDeviceToHost));
  h.epoch = e->state_epoch;
  h.wm = e->cur_wm;
  return FW_OK;
}

// restored purged sessions' cleanup timers the watermark has reached: each fetched its key's set when it fired
// (onEventTime -> getMergingWindowSet), at the ordinal of the advance that reached it.  The ones still pending lie
// ahead of every advance so far, so only the last advance is kept
static void session_fire_rorphans(fw_engine* e) {
  const int64_t lateness = e->cfg.allowed_lateness;
  for (auto it = e->sess_rorphans.begin(); it != e->sess_rorphans.end();) {
    const int64_t ct = fw::cleanup_time(fw::jsub((*it)[2], 1), lateness);
    if (ct > e->cur_wm) { ++it; continue; }
    int64_t ord = 0;
    for (const auto& a : e->sess_adv) if (a.first >= ct) { ord = a.second; break; }
    auto adj = e->sess_touch_adj.find((*it)[0]);
    if (adj == e->sess_touch_adj.end() || std::make_pair(ord, ct) < adj->second) e->sess_touch_adj[(*it)[0]] = {ord, ct};
    it = e->sess_rorphans.erase(it);
  }
  if (e->sess_adv.size() > 1) e->sess_adv.erase(e->sess_adv.begin(), e->sess_adv.end() - 1);
}

static int session_reject_config(fw_engine* e) {
  if (!e->sess.ckpt)
    return reject(e, FW_ERR_UNSUPPORTED, "session checkpoint bookkeeping is off (FW_SESS_CKPT=0)");
  if (e->mws_created.empty()) e->mws_created.assign((size_t)(e->s.kg_end - e->s.kg_start + 1), 0);
  if (e->kg_touched.empty()) e->kg_touched.assign((size_t)(e->s.kg_end - e->s.kg_start + 1), 0);
  return FW_OK;
}

static int session_snapshot_kg_flink(fw_engine* e, int32_t kg, const fw_state_layout* layout, void* state,
                                     int64_t state_cap, int64_t* state_len, void* timers, int64_t timers_cap,
                                     int64_t* timers_len) {
  if (int rc = session_reject_config(e)) return rc;
  HIPCHK(e, hipSetDevice(e->dev));
  if (int rc = session_download(e)) return rc;
  const fw_engine::SessHost& h = e->sess_host;
  const fw::Spec& s = e->s;
  const SessDev& d = e->sess;
  const fw_config& c = e->cfg;
  const size_t kgi = (size_t)(kg - s.kg_start);
  const bool orphans = c.trigger == FW_TRIGGER_PURGING_EVENT_TIME && c.allowed_lateness > 0;
  if (h.nslog_over)
    return reject(e, FW_ERR_CAPACITY, "the shared-namespace log overflowed: the order of a namespace still live is unknown until it ends");
  if (orphans) {   // purged sessions' cleanup timers logged since the last snapshot (or the log's last pruning)
    unsigned long long no = 0;
    long long lost = INT64_MIN;
    HIPCHK(e, hipMemcpy(&no, d.olog_n, 8, hipMemcpyDeviceToHost));
    HIPCHK(e, hipMemcpy(&lost, d.lmeta + LM_OLOST, 8, hipMemcpyDeviceToHost));
    const size_t take = (size_t)std::min<int64_t>((int64_t)no, d.olog_cap);   // (entries past the cap were dropped)
    std::vector<int64_t> ol(4 * take);
    if (take) HIPCHK(e, hipMemcpy(ol.data(), d.olog, 8 * ol.size(), hipMemcpyDeviceToHost));
    HIPCHK(e, hipMemset(d.olog_n, 0, 8));
    e->sess_olog_drained += (int64_t)no;
    for (size_t j = 0; j < take; ++j) e->sess_orphans.push_back({ol[4 * j], ol[4 * j + 1], ol[4 * j + 2], ol[4 * j + 3]});
    auto ct_of = [&](int64_t end) { return fw::cleanup_time(fw::jsub(end, 1), c.allowed_lateness); };
    std::vector<std::array<int64_t, 4>> keep;
    for (const auto& o : e->sess_orphans) if (ct_of(o[2]) > e->cur_wm) keep.push_back(o);
    e->sess_orphans.swap(keep);
    session_fire_rorphans(e);
    // (intended ahead of the rejection: the drained entries are kept in sess_orphans, nothing is lost by a failing
    // snapshot, and the log has room again)
    // a dropped entry's timer is missing from the timers below until the watermark reaches it
    if ((int64_t)lost > e->cur_wm)
      return reject(e, FW_ERR_CAPACITY, "more purged sessions' cleanup timers pending than the orphan timer log holds (snapshots succeed again once the watermark passes the dropped ones)");
  }
  struct Pane { int64_t kid, key, start, end, sws, swc, put, cre, tre; bool trig; KgPane acc; int64_t lhead, llen; };
  std::vector<Pane> panes;
  int64_t n_touched = 0;
  bool any_acc = false, kg_acc = false;
  // when a key's set was first fetched: the device's record or watermark, or a restored timer's firing (host)
  auto touch_of = [&](int64_t kid, int64_t key) -> std::pair<int64_t, int64_t> {
    std::pair<int64_t, int64_t> t{h.ktouch[(size_t)kid], h.ktts[(size_t)kid]};
    auto adj = e->sess_touch_adj.find(key);
    if (adj != e->sess_touch_adj.end() && (t.first < 0 || adj->second < t)) t = adj->second;
    return t;
  };
  std::set<int64_t> dir_keys_touched;
  for (int64_t k = 0; k < s.stride; ++k) {
    const int64_t key = k == s.D ? fw::EMPTY_KEY : h.keys[(size_t)k];
    if (k < s.D && key == fw::EMPTY_KEY) continue;
    if (touch_of(k, key).first >= 0) { ++n_touched; dir_keys_touched.insert(key); }
    any_acc = any_acc || h.kacc[(size_t)k];
    if (host_key_group(s, key) != kg) continue;
    kg_acc = kg_acc || h.kacc[(size_t)k];
    for (int q = 0; q < d.sw; ++q) {
      const size_t w = (size_t)k * (size_t)d.nw + (size_t)(q >> 6);
      if (!((h.live[w] >> (q & 63)) & 1ull)) continue;
      const size_t x = (size_t)k * (size_t)d.sw + (size_t)q;
      Pane p{k, key, h.st[x], h.en[x], h.sws[x], h.swc[x], h.put[x], h.cre[x], h.tre[x], ((h.trig[w] >> (q & 63)) & 1ull) != 0, {},
             h.lhead.empty() ? -1 : h.lhead[x], h.llen.empty() ? 0 : h.llen[x]};
      p.acc = KgPane{p.sws, fw::jadd(p.sws, d.gap), key, h.sum.empty() ? 0 : h.sum[x], h.mn.empty() ? INT64_MAX : h.mn[x],
                     h.mx.empty() ? INT64_MIN : h.mx[x], h.cnt.empty() ? 0 : h.cnt[x], 0, h.f1.empty() ? 0 : h.f1[x], false};
      panes.push_back(p);
    }
  }
  for (const auto& a : e->sess_touch_adj) if (!dir_keys_touched.count(a.first)) ++n_touched;   // (keys not in the directory)
  const bool wc_table = e->sess_wc_table || any_acc;
  const bool mws_table = e->sess_mws_table || n_touched > 0;
  fwkg::BeOut st;
  if (wc_table || mws_table) st.i32(kg);
  int id = 0;
  if (wc_table) {   // "window-contents": namespaces = state windows, created by their first record
    const bool present = kg_acc || e->kg_touched[kgi];
    st.i16(id++);
    st.u8(present ? 1 : 0);
    if (present) {
      std::vector<fwkg::WcNamespace> nsv = fwkg::group_namespaces(
          panes.size(), [&](size_t i) { return std::make_pair(panes[i].sws, fw::jadd(panes[i].sws, d.gap)); });
      // when each namespace's current instance was put into the namespace map: its entries' lifetimes — the live
      // ones and the logged entries of other keys removed while it stayed shared — chained without a gap
      std::map<int64_t, std::vector<std::pair<int64_t, int64_t>>> life;
      for (const auto& w : nsv) life[w.start];
      for (size_t j = 0; j + 4 <= h.nslog.size(); j += 4)
        if (life.count(h.nslog[j + 1]) && host_key_group(s, h.nslog[j]) == kg) life[h.nslog[j + 1]].push_back({h.nslog[j + 2], h.nslog[j + 3]});
      std::vector<int64_t> ns_first(nsv.size(), INT64_MAX);
      for (size_t w = 0; w < nsv.size(); ++w) {
        auto& iv = life[nsv[w].start];
        for (size_t i : nsv[w].entries) iv.push_back({panes[i].swc, INT64_MAX});
        std::sort(iv.begin(), iv.end());
        int64_t from = iv[0].first, reach = iv[0].second;
        for (const auto& x : iv) {
          if (x.first >= reach) from = x.first;   // a gap: the namespace was removed and put again
          reach = x.first >= reach ? x.second : std::max(reach, x.second);
        }
        ns_first[w] = from;
      }
      fwkg::write_window_contents(
          st, wc_layout(e, layout), nsv,
          [&](size_t a, size_t b) { return ns_first[a] != ns_first[b] ? ns_first[a] < ns_first[b] : nsv[a].start < nsv[b].start; },
          [&](size_t i) { return panes[i].key; },
          [&](size_t a, size_t b) { return panes[a].swc != panes[b].swc ? panes[a].swc < panes[b].swc : panes[a].key < panes[b].key; },
          [&](size_t i, fwkg::WcEntry& ent) {
            if (!d.list) return pane_words(e, layout, panes[i].acc, ent.word);
            int64_t el = panes[i].lhead;   // the window's elements in list order
            for (int64_t j = 0; j < panes[i].llen && el >= 0 && el < d.pcap; ++j, el = h.pnext[(size_t)el])
              ent.el.push_back({value_word(e, h.pv[(size_t)el]), h.pf1[(size_t)el]});
          });
    }
  }
  if (mws_table) {   // "merging-window-set", as WindowOperator.snapshotState rewrites it
    // entries: the restored ones of keys not touched since (inserted at the restore, in blob order), then every
    // other key with sessions in flight, re-added in mergingWindowsByKey's order (HashMap<K, MergingWindowSet>
    // over every key fetched since the operator opened: bucket, then first fetch)
    struct Ent { int64_t kid, key, rank; bool touched; std::vector<size_t> slots; };
    std::vector<Ent> ents;
    std::map<int64_t, size_t> at;
    for (size_t i = 0; i < panes.size(); ++i) {
      auto it = at.find(panes[i].kid);
      if (it == at.end()) {
        const int64_t k = panes[i].kid;
        auto r = e->sess_mws_rank.find(panes[i].key);
        const bool touched = touch_of(k, panes[i].key).first >= 0 || r == e->sess_mws_rank.end();
        it = at.emplace(k, ents.size()).first;
        ents.push_back({k, panes[i].key, touched ? INT64_MAX : r->second, touched, {}});
      }
      ents[it->second].slots.push_back(i);
    }
    if (!ents.empty()) e->mws_created[kgi] = 1;
    const bool present = e->mws_created[kgi] != 0;
    st.i16(id++);
    st.u8(present ? 1 : 0);
    if (present) {
      st.i32(ents.empty() ? 0 : 1);
      if (!ents.empty()) {
        st.u8(0);   // VoidNamespaceSerializer: one byte
        const uint32_t gmask = fwkg::capacity_for((size_t)n_touched) - 1;
        std::vector<size_t> eo(ents.size());
        for (size_t i = 0; i < eo.size(); ++i) eo[i] = i;
        fwkg::hashmap_order(
            eo, [&](size_t i) { return fw::long_hash_code(ents[i].key); },
            [&](size_t a, size_t b) {
              const Ent &x = ents[a], &y = ents[b];
              if (x.touched != y.touched) return !x.touched;
              if (!x.touched) return x.rank < y.rank;
              const uint32_t gx = (uint32_t)fwkg::spread(fw::long_hash_code(x.key)) & gmask;
              const uint32_t gy = (uint32_t)fwkg::spread(fw::long_hash_code(y.key)) & gmask;
              if (gx != gy) return gx < gy;
              const auto tx = touch_of(x.kid, x.key), ty = touch_of(y.kid, y.key);
              return tx != ty ? tx < ty : x.key < y.key;
            });
        st.i32((int32_t)ents.size());
        for (size_t i : eo) {
          std::vector<size_t>& sl = ents[i].slots;   // MergingWindowSet.windows (HashMap<W, W>): bucket, then put order
          fwkg::hashmap_order(
              sl, [&](size_t j) { return fwkg::window_hash(panes[j].start, panes[j].end); },
              [&](size_t a, size_t b) { return panes[a].put < panes[b].put; });
          st.i64(ents[i].key);
          st.i32((int32_t)sl.size());
          for (size_t j : sl) {
            st.i64(panes[j].start);
            st.i64(panes[j].end);
            st.i64(panes[j].sws);
            st.i64(fw::jadd(panes[j].sws, d.gap));
          }
        }
      }
    }
  }
  // timers: per in-flight window its trigger timer while pending (registered by onElement / onMerge) and its
  // cleanup timer (registerCleanupTimer right after; one timer when the lateness is 0); restored ones keep their
  // blob order ahead of every later one
  struct Tm { int64_t key, start, end, ts, seq; int kind; };
  std::vector<Tm> tv;
  for (const Pane& p : panes) {
    const int64_t max_ts = fw::jsub(p.end, 1), ct = fw::cleanup_time(max_ts, c.allowed_lateness);
    if (p.trig) tv.push_back({p.key, p.start, p.end, max_ts, p.tre, 0});
    if (ct != max_ts) tv.push_back({p.key, p.start, p.end, ct, p.cre, 1});
  }
  if (orphans) {   // purged sessions' cleanup timers (the same timer as a later in-flight window's keeps its place)
    std::map<std::array<int64_t, 3>, size_t> at;
    for (size_t i = 0; i < tv.size(); ++i) if (tv[i].kind == 1) at[{tv[i].key, tv[i].start, tv[i].end}] = i;
    auto add = [&](int64_t key, int64_t start, int64_t end, int64_t seq) {
      if (host_key_group(s, key) != kg) return;
      auto it = at.find({key, start, end});
      if (it != at.end()) { tv[it->second].seq = std::min(tv[it->second].seq, seq); return; }
      at[{key, start, end}] = tv.size();
      tv.push_back({key, start, end, fw::cleanup_time(fw::jsub(end, 1), c.allowed_lateness), seq, 1});
    };
    for (const auto& o : e->sess_rorphans) add(o[0], o[1], o[2], INT64_MIN);
    for (const auto& o : e->sess_orphans) add(o[0], o[1], o[2], o[3]);
  }
  return finish_sections(
      e, st, tv.size(), [&](size_t i) { return fwkg::Timer{tv[i].key, tv[i].start, tv[i].end, tv[i].ts}; },
      [&](size_t a, size_t b) { return tv[a].seq != tv[b].seq ? tv[a].seq < tv[b].seq : tv[a].kind < tv[b].kind; },
      state, state_cap, state_len, timers, timers_cap, timers_len);
}

static int session_restore_kg_flink(fw_engine* e, int32_t kg, const fw_state_layout* layout, int64_t watermark,
                                    const void* state, int64_t state_len, const void* timers, int64_t timers_len) {
  if (int rc = session_reject_config(e)) return rc;
  const fw::Spec& s = e->s;
  const SessDev& d = e->sess;
  const fw_config& c = e->cfg;
  const size_t kgi = (size_t)(kg - s.kg_start);
  struct WcEnt { KgPane p; int64_t rank; std::vector<std::array<int64_t, 2>> el; };   // (list state: value, f1)
  std::map<std::pair<int64_t, int64_t>, WcEnt> wc;   // (state-window start, key) -> its state
  std::vector<std::pair<int64_t, std::vector<std::array<int64_t, 4>>>> mws;
  bool wc_seen = false, mws_seen = false, wc_present = false, mws_present = false;
  if (state_len > 0) {
    fwkg::BeIn in(state, state_len);
    if (in.i32() != kg) return reject(e, FW_ERR_INVALID_ARG, "state section of another key group");
    for (int table = 0; in.ok && (table == 0 || in.pos < in.n); ++table) {   // (at least one table)
      if (in.i16() != table || table > 1) return reject(e, FW_ERR_UNSUPPORTED, "keyed state other than window-contents and merging-window-set");
      const bool present = in.u8() != 0;
      if (table == 0) {
        wc_seen = true;
        wc_present = present;
        int rc = FW_OK;
        const fwkg::WcFail f = !present ? fwkg::WcFail::none : fwkg::read_window_contents(
            in, wc_layout(e, layout),
            [&](int64_t start, int64_t end) {
              if (end != fw::jadd(start, d.gap))
                rc = reject(e, FW_ERR_INVALID_ARG, "namespace is not a state window [ts, ts + gap) of this assigner");
              return rc == FW_OK;
            },
            [&](int64_t start, int64_t end, fwkg::WcEntry& ent) {
              KgPane p{start, end, ent.key, 0, INT64_MAX, INT64_MIN, 0, 0, 0, false};
              pane_from_words(e, layout, ent.word, p);
              if (host_key_group(s, p.key) != kg) rc = reject(e, FW_ERR_KEY_GROUP, "state entry key outside its key group");
              else if (!wc.emplace(std::make_pair(start, p.key), WcEnt{p, e->restore_ord++, std::move(ent.el)}).second)
                rc = reject(e, FW_ERR_INVALID_ARG, "duplicate (window, key) entry");
              return rc == FW_OK;
            });
        if (f == fwkg::WcFail::stopped) return rc;
        if (f != fwkg::WcFail::none) return reject_state(e, f);
      } else {
        mws_seen = true;
        mws_present = present;
        const int32_t nns = present ? in.i32() : 0;
        if (nns < 0 || nns > 1) return reject(e, FW_ERR_INVALID_ARG, "corrupt merging-window-set section");
        if (nns == 1 && in.u8() != 0) return reject(e, FW_ERR_INVALID_ARG, "merging-window-set namespace is not VoidNamespace");
        const int32_t ne = nns ? in.i32() : 0;
        if (ne < 0) return reject(e, FW_ERR_INVALID_ARG, "corrupt merging-window-set section");
        for (int32_t j = 0; j < ne && in.ok; ++j) {
          const int64_t key = in.i64();
          const int32_t m = in.i32();
          if (m < 0) return reject(e, FW_ERR_INVALID_ARG, "corrupt merging-window-set entry");
          if (m > d.sw) return reject(e, FW_ERR_CAPACITY, "more in-flight sessions for a key than max_open_slices");
          std::vector<std::array<int64_t, 4>> l;
          for (int32_t q = 0; q < m && in.ok; ++q) l.push_back({in.i64(), in.i64(), in.i64(), in.i64()});
          if (!in.ok) break;
          if (host_key_group(s, key) != kg) return reject(e, FW_ERR_KEY_GROUP, "merging-window-set key outside its key group");
          mws.push_back({key, std::move(l)});
        }
      }
    }
    if (!in.done()) return reject(e, FW_ERR_INVALID_ARG, "state section truncated or with trailing bytes");
  }
  std::vector<fwkg::Timer> got;
  if (int rc = read_timer_section(e, timers, timers_len, got)) return rc;
  // the in-flight windows: each with its state window's contents; timers exactly the ones they imply
  std::set<fwkg::Timer> tset(got.begin(), got.end()), want;
  std::vector<int64_t> rows;
  std::vector<std::array<int64_t, 4>> pool;   // list state: (entry, value, f1, next)
  std::set<std::pair<int64_t, int64_t>> used, keys_seen;
  for (const auto& kv : mws) {
    if (!keys_seen.insert({kv.first, 0}).second) return reject(e, FW_ERR_INVALID_ARG, "duplicate merging-window-set key");
    for (size_t q = 0; q < kv.second.size(); ++q) {
      const auto& w = kv.second[q];   // window start, end, state window start, end
      if (w[3] != fw::jadd(w[2], d.gap) || w[0] > w[2] || w[1] < w[3])
        return reject(e, FW_ERR_INVALID_ARG, "a state window is not a session's first window inside the window");
      auto it = wc.find({w[2], kv.first});
      if (it == wc.end()) return reject(e, FW_ERR_INVALID_ARG, "in-flight session without window-contents state");
      used.insert({w[2], kv.first});
      const int64_t max_ts = fw::jsub(w[1], 1), ct = fw::cleanup_time(max_ts, c.allowed_lateness);
      const fwkg::Timer trig_t{kv.first, w[0], w[1], max_ts};
      const bool trig = tset.count(trig_t) != 0;
      if (trig) want.insert(trig_t);
      if (ct != max_ts) want.insert(fwkg::Timer{kv.first, w[0], w[1], ct});
      const KgPane& p = it->second.p;
      int64_t lh = -1, lt = -1, ln = 0;
      if (e->list) {   // the elements into pool entries, chained in list order
        const auto& el = it->second.el;
        if (e->sess_pool_used + (int64_t)el.size() > d.pcap)
          return reject(e, FW_ERR_CAPACITY, "restored session elements exceed list_capacity");
        lh = e->sess_pool_used;
        for (size_t j = 0; j < el.size(); ++j) {
          const int64_t at = e->sess_pool_used++;
          pool.push_back({at, el[j][0], el[j][1], j + 1 < el.size() ? at + 1 : -1});
        }
        lt = e->sess_pool_used - 1;
        ln = (int64_t)el.size();
      }
      const int64_t row[fw::SESS_ROW] = {kv.first, (int64_t)q, w[0], w[1], w[2], it->second.rank,
                                         trig ? 1 : 0, p.sum, p.mn, p.mx, p.cnt, p.f1, lh, lt, ln};
      rows.insert(rows.end(), row, row + fw::SESS_ROW);
    }
  }
  if (used.size() != wc.size()) return reject(e, FW_ERR_INVALID_ARG, "window-contents state of no in-flight session");
  if (!std::includes(tset.begin(), tset.end(), want.begin(), want.end()))
    return reject(e, FW_ERR_UNSUPPORTED, "timers differ from the ones the sessions imply");
  std::vector<std::array<int64_t, 3>> rorph;   // PurgingTrigger + lateness: cleanup timers of purged sessions
  for (const auto& t : tset) {
    if (want.count(t)) continue;
    const int64_t max_ts = fw::jsub(t.end, 1), ct = fw::cleanup_time(max_ts, c.allowed_lateness);
    if (c.trigger != FW_TRIGGER_PURGING_EVENT_TIME || ct == max_ts || t.ts != ct || t.end <= t.start ||
        host_key_group(s, t.key) != kg)
      return reject(e, FW_ERR_UNSUPPORTED, "timers differ from the ones the sessions imply");
    rorph.push_back({t.key, t.start, t.end});
    e->sess_rorph_ct = std::max(e->sess_rorph_ct, ct);
  }
  HIPCHK(e, hipSetDevice(e->dev));
  for (const auto& kv : mws) e->sess_mws_rank[kv.first] = (int64_t)e->sess_mws_rank.size();
  e->sess_rorphans.insert(rorph.begin(), rorph.end());
  if (e->sess_adv.empty()) e->sess_adv.push_back({watermark, 0});
  for (const auto& t : got) e->restored_timer_rank[t] = (int64_t)e->restored_timer_rank.size();
  if (wc_seen) e->sess_wc_table = true;
  if (mws_seen) e->sess_mws_table = true;
  if (wc_present) e->kg_touched[kgi] = 1;
  if (mws_present) e->mws_created[kgi] = 1;
  e->restored = true;
  e->cur_wm = watermark;
  e->state_epoch++;
  if (!pool.empty()) {   // the entries the restored elements took (the pool's free ring hands out the rest)
    std::vector<int64_t> pv(pool.size()), pf(pool.size()), pn(pool.size());
    const int64_t first = pool[0][0];
    for (size_t j = 0; j < pool.size(); ++j) { pv[j] = pool[j][1]; pf[j] = pool[j][2]; pn[j] = pool[j][3]; }
    HIPCHK(e, hipMemcpy(d.pv + first, pv.data(), 8 * pv.size(), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(d.pf1 + first, pf.data(), 8 * pf.size(), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(d.pnext + first, pn.data(), 8 * pn.size(), hipMemcpyHostToDevice));
    const unsigned long long taken = (unsigned long long)e->sess_pool_used;
    HIPCHK(e, hipMemcpy(d.pool, &taken, 8, hipMemcpyHostToDevice));
  }
  const int64_t n = (int64_t)(rows.size() / fw::SESS_ROW);
  if (n == 0) return FW_OK;
  return launch_on_rows(e, rows.data(), rows.size(), [&](int64_t* dr) {
    hipLaunchKernelGGL(fw::k_sess_restore, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, e->stream, e->s,
                       e->sess, dr, n, -((int64_t)1 << 61));
  });
}

static int window_snapshot_kg_flink(fw_engine* e, int32_t kg, const fw_state_layout* layout, void* state,
                                    int64_t state_cap, int64_t* state_len, void* timers, int64_t timers_cap,
                                    int64_t* timers_len) {
  const fw_config& c = e->cfg;
  const bool sl_purge = c.trigger == FW_TRIGGER_PURGING_EVENT_TIME && c.allowed_lateness > 0 && c.assigner == FW_SLIDING;
  if (sl_purge && !e->s.first)
    return reject(e, FW_ERR_UNSUPPORTED, "sliding windows under PurgingTrigger with allowed lateness need first-arrival "
                                         "tracking (keep_first_f1) to tell which keys' cleanup timers outlive a purge");
  HIPCHK(e, hipSetDevice(e->dev));
  if (int rc = build_snapshot(e)) return rc;
  std::vector<KgPane> panes;
  kg_panes(e, kg, panes);
  struct Ghost { int64_t key, start, end, first; };
  std::vector<Ghost> sl_ghosts;
  if (sl_purge) {   // fired windows: no state (FIRE_AND_PURGE); cleanup timers of the keys that had an element before
    std::vector<KgPane> kept;
    std::set<std::pair<int64_t, int64_t>> seen;
    for (const KgPane& p : panes) {
      const int64_t max_ts = fw::jsub(p.end, 1);
      if (max_ts > e->cur_wm) { kept.push_back(p); continue; }
      int64_t fire_ord = 0;   // the arrival ordinal at the advance that fired the window (or the restore)
      for (const auto& a : e->adv_log) if (a.first >= max_ts) { fire_ord = a.second; break; }
      if (p.first + e->ordinal < fire_ord && seen.insert({p.start, p.key}).second) sl_ghosts.push_back({p.key, p.start, p.end, p.first});
    }
    for (const auto& g : e->sl_ghost) {   // restored ones
      const int64_t end = fw::jadd(g.first, c.size);
      if (fw::cleanup_time(fw::jsub(end, 1), c.allowed_lateness) <= e->cur_wm || host_key_group(e->s, g.second) != kg) continue;
      if (seen.insert({g.first, g.second}).second) sl_ghosts.push_back({g.second, g.first, end, INT64_MIN});
    }
    panes.swap(kept);
  }
  const bool first = e->s.first;
  bool any_state = e->snap_any_key;
  for (uint8_t t : e->kg_touched) any_state = any_state || t;
  fwkg::BeOut st;
  if (any_state) {
    const bool present = !panes.empty() || e->snap_has_key[(size_t)kg] ||
                         (!e->kg_touched.empty() && e->kg_touched[(size_t)(kg - e->s.kg_start)]);
    st.i32(kg);
    st.i16(0);
    st.u8(present ? 1 : 0);
    if (present) {
      // namespaces: HashMap<TimeWindow, HashMap<K, S>>, created by the first arrival into the window
      // namespaces: HashMap<TimeWindow, HashMap<K, S>>, created by the first arrival into the window
      std::vector<fwkg::WcNamespace> nsv =
          fwkg::group_namespaces(panes.size(), [&](size_t i) { return std::make_pair(panes[i].start, panes[i].end); });
      std::vector<int64_t> ns_first(nsv.size(), INT64_MAX);
      for (size_t w = 0; w < nsv.size(); ++w)
        for (size_t i : nsv[w].entries) ns_first[w] = std::min(ns_first[w], panes[i].first);
      fwkg::write_window_contents(
          st, wc_layout(e, layout), nsv,
          [&](size_t a, size_t b) {   // (nsv ascends by (start, end))
            return first && ns_first[a] != ns_first[b] ? ns_first[a] < ns_first[b] : a < b;
          },
          [&](size_t i) { return panes[i].key; },
          [&](size_t a, size_t b) {
            return first && panes[a].first != panes[b].first ? panes[a].first < panes[b].first : panes[a].key < panes[b].key;
          },
          [&](size_t i, fwkg::WcEntry& ent) {
            if (!e->list) return pane_words(e, layout, panes[i], ent.word);
            // ListSerializer.serialize: every element in insertion order (sliding: the window's list holds its
            // slices' elements of the key, merged in arrival order)
            std::vector<std::array<int64_t, 3>> merged;
            if (c.assigner == FW_SLIDING) {
              const int64_t n = fw::floor_div(fw::jsub(panes[i].start, c.offset), c.slide);
              for (int64_t mm = n * e->s.R; mm < n * e->s.R + e->s.K; ++mm) {
                auto it = e->snap_list.find({mm, panes[i].key});
                if (it != e->snap_list.end()) merged.insert(merged.end(), it->second.begin(), it->second.end());
              }
              std::sort(merged.begin(), merged.end());
            }
            const auto& el = c.assigner == FW_SLIDING ? merged : e->snap_list.at({panes[i].m, panes[i].key});
            for (const auto& x : el) ent.el.push_back({value_word(e, x[1]), x[2]});
          });
    }
  }
  // timers: per pane the trigger timer at maxTimestamp while it has not fired, and the cleanup timer (the
  // same timer when the lateness is 0), registered in that order by the pane's first arrival
  // (WindowOperator.java:314-330; EventTimeTrigger.onElement :37-45); a record's sliding windows register
  // theirs latest window first (SlidingEventTimeWindows.assignWindows :64-77)
  // (restored timers: added at restore, before any later one, in the order of the restored sections)
  struct Tm { int64_t key, start, end, ts, first; int kind; };
  std::vector<Tm> tv;
  for (const KgPane& p : panes) {
    const int64_t max_ts = fw::jsub(p.end, 1), ct = fw::cleanup_time(max_ts, c.allowed_lateness);
    if (max_ts > e->cur_wm && !p.unarmed) tv.push_back({p.key, p.start, p.end, max_ts, p.first, 0});
    if (ct != max_ts || max_ts <= e->cur_wm) tv.push_back({p.key, p.start, p.end, ct, p.first, 1});
  }
  for (const Ghost& g : sl_ghosts)
    tv.push_back({g.key, g.start, g.end, fw::cleanup_time(fw::jsub(g.end, 1), c.allowed_lateness), g.first, 1});
  // purged windows' cleanup timers (no state; a key whose window holds state again has the timer above)
  if (!e->snap_gkg.empty()) {
    std::set<std::pair<int64_t, int64_t>> has;
    for (const KgPane& p : panes) has.insert({p.start, p.key});
    const std::vector<int64_t>& g = e->snap_gkg[(size_t)kg];
    for (size_t j = 0; j + 3 <= g.size(); j += 3) {
      const int64_t start = host_window_start(c, g[j]), end = fw::jadd(start, c.size);
      if (has.count({start, g[j + 1]})) continue;
      tv.push_back({g[j + 1], start, end, fw::cleanup_time(fw::jsub(end, 1), c.allowed_lateness), g[j + 2], 1});
    }
  }
  return finish_sections(
      e, st, tv.size(), [&](size_t i) { return fwkg::Timer{tv[i].key, tv[i].start, tv[i].end, tv[i].ts}; },
      [&](size_t a, size_t b) {
        const Tm &x = tv[a], &y = tv[b];
        if (first && x.first != y.first) return x.first < y.first;
        if (!first && x.key != y.key) return x.key < y.key;
        if (x.start != y.start) return x.start > y.start;
        return x.kind < y.kind;
      },
      state, state_cap, state_len, timers, timers_cap, timers_len);
}

extern "C" int fw_snapshot_kg_flink(fw_engine* e, int32_t kg, const fw_state_layout* layout, void* state,
                                    int64_t state_cap, int64_t* state_len, void* timers, int64_t timers_cap,
                                    int64_t* timers_len) {
  if (!e || !state_len || !timers_len) return FW_ERR_INVALID_ARG;
  if (e->sticky) return e->sticky;
  if (kg < e->s.kg_start || kg > e->s.kg_end)
    return reject(e, FW_ERR_INVALID_ARG, "Key Group " + std::to_string(kg) + " does not belong to the local range.");
  if (e->used_key_hash) return reject(e, FW_ERR_UNSUPPORTED, "snapshot needs Long keys (a push carried Java key hashes)");
  if (int rc = check_state_layout(e, layout)) return rc;
  return (e->session ? session_snapshot_kg_flink : window_snapshot_kg_flink)(e, kg, layout, state, state_cap, state_len,
                                                                             timers, timers_cap, timers_len);
}

// list state: restored elements appended to their slices' buffers (the directory and the slots were set by
// restore_entries).  each(add) calls add(slice, key, ordinal, value, f1) once per element
template <class Each>
static int append_list_elements(fw_engine* e, Each each) {
  const fw::Spec& s = e->s;
  std::vector<int64_t> keys((size_t)s.D);
  HIPCHK(e, hipMemcpy(keys.data(), s.dir_keys, 8 * (size_t)s.D, hipMemcpyDeviceToHost));
  std::unordered_map<int64_t, int64_t> kid_of;
  for (int64_t k = 0; k < s.D; ++k) if (keys[(size_t)k] != fw::EMPTY_KEY) kid_of[keys[(size_t)k]] = k;
  std::vector<unsigned long long> lc((size_t)s.P);
  HIPCHK(e, hipMemcpy(lc.data(), e->lst.cnt, 8 * (size_t)s.P, hipMemcpyDeviceToHost));
  std::map<int32_t, std::vector<int64_t>> rows;   // slot -> elements (kid, ordinal, value, f1)
  bool unknown_key = false;
  each([&](int64_t slice, int64_t key, int64_t ord, int64_t value, int64_t f1) {
    const int64_t kid = key == fw::EMPTY_KEY ? s.D : (kid_of.count(key) ? kid_of[key] : -1);
    auto& r = rows[(int32_t)fw::floor_mod(slice, s.P)];
    r.insert(r.end(), {kid, ord, value, f1});
    unknown_key = unknown_key || kid < 0;
  });
  if (unknown_key) return reject(e, FW_ERR_CAPACITY, "restored key not in the key directory");
  for (auto& kv : rows) {
    const int32_t p = kv.first;
    const int64_t n = (int64_t)(kv.second.size() / LST_WORDS);
    if ((int64_t)lc[(size_t)p] + n > e->lst.cap)
      return reject(e, FW_ERR_CAPACITY, "restored list state exceeds list_capacity for its slice");
    HIPCHK(e, hipMemcpy(e->lst.buf + ((size_t)p * (size_t)e->lst.cap + lc[(size_t)p]) * LST_WORDS, kv.second.data(),
                        8 * kv.second.size(), hipMemcpyHostToDevice));
    lc[(size_t)p] += (unsigned long long)n;
  }
  HIPCHK(e, hipMemcpy(e->lst.cnt, lc.data(), 8 * (size_t)s.P, hipMemcpyHostToDevice));
  e->state_epoch++;
  return FW_OK;
}

// Sliding-window list state (slide dividing the size: a slice per slide, window n = slices n .. n + K - 1): the
// reference holds each window's list; the engine holds each record once, in its slice.  Per key, the windows are
// peeled newest first: window n's list, less the elements of slices n + 1 .. n + K - 1 (known from the newer
// windows, matched in order as a subsequence), is slice n; its elements join the key's arrival order right after
// the element they follow in the list.  Every window's list is then rebuilt from the slices and checked; the
// elements get ordinals in that arrival order, ahead of every later record
static int restore_sliding_lists(fw_engine* e, int64_t wm, const std::vector<KgPane>& panes, const std::vector<int64_t>& win,
                                 const std::vector<std::vector<std::array<int64_t, 2>>>& lists) {
  const fw::Spec& s = e->s;
  const int64_t K = s.K;
  std::map<int64_t, std::map<int64_t, size_t>> by_key;   // key -> window -> entry
  for (size_t i = 0; i < panes.size(); ++i) {
    by_key[panes[i].key][win[i]] = i;
    e->list_entry_rank[{panes[i].start, panes[i].key}] = e->restore_ord++;
  }
  struct El { int64_t v, f1, m; };
  std::map<std::pair<int64_t, int64_t>, std::vector<std::array<int64_t, 3>>> slices;   // (slice, key) -> (ord, v, f1)
  const int64_t R = s.R;
  // the oldest window still in its lifetime at wm (every newer one exists once a record of its slices arrived)
  int64_t n_alive = INT64_MIN / 4;
  if (wm != INT64_MIN) {
    const __int128 x = (__int128)wm - e->cfg.allowed_lateness - e->cfg.offset - e->cfg.size + 1;
    const __int128 sl = e->cfg.slide;
    __int128 q = x / sl;
    if (x % sl != 0 && x < 0) --q;
    n_alive = (int64_t)std::max<__int128>(q + 1, (__int128)(INT64_MIN / 4));
  }
  for (const auto& kw : by_key) {
    const int64_t key = kw.first;
    const auto& wins = kw.second;
    std::vector<El> order;
    if (R != 1) {
      // a slide that does not divide the size: each element (distinct within a window) is identified across the
      // windows' lists; its live windows [lo, hi] pick a slice m with floor(m / R) = hi whose oldest live window is
      // lo; the arrival order is any order every list agrees with (a topological order of their successions)
      std::map<std::pair<int64_t, int64_t>, int64_t> id;
      std::vector<El> el;
      std::vector<std::pair<int64_t, int64_t>> span;   // (lo, hi) of windows holding the element
      std::vector<int64_t> nwin;
      std::vector<std::vector<int64_t>> seqs;
      for (const auto& w : wins) {
        std::set<int64_t> seen;
        std::vector<int64_t> seq;
        for (const auto& x : lists[w.second]) {
          auto it = id.find({x[0], x[1]});
          int64_t k;
          if (it == id.end()) {
            k = (int64_t)el.size();
            id[{x[0], x[1]}] = k;
            el.push_back({x[0], x[1], 0});
            span.push_back({w.first, w.first});
            nwin.push_back(0);
          } else {
            k = it->second;
          }
          if (!seen.insert(k).second)
            return reject(e, FW_ERR_UNSUPPORTED, "sliding-window lists with equal elements (slide not dividing the size)");
          span[(size_t)k].first = std::min(span[(size_t)k].first, w.first);
          span[(size_t)k].second = std::max(span[(size_t)k].second, w.first);
          nwin[(size_t)k]++;
          seq.push_back(k);
        }
        seqs.push_back(std::move(seq));
      }
      for (size_t k = 0; k < el.size(); ++k) {
        const int64_t lo = span[k].first, hi = span[k].second;
        if (nwin[k] != hi - lo + 1) return reject(e, FW_ERR_INVALID_ARG, "an element missing from a window between its windows");
        bool found = false;
        for (int64_t m = hi * R; m < hi * R + R && !found; ++m) {
          const int64_t first_w = fw::floor_div(m - K + 1 + R - 1, R);
          if (std::max(first_w, n_alive) == lo) { el[k].m = m; found = true; }
        }
        if (!found) return reject(e, FW_ERR_INVALID_ARG, "an element's windows are not those of any slice");
      }
      std::vector<std::vector<int64_t>> succ(el.size());
      std::vector<int64_t> indeg(el.size(), 0);
      for (const auto& seq : seqs)
        for (size_t j = 1; j < seq.size(); ++j) { succ[(size_t)seq[j - 1]].push_back(seq[j]); indeg[(size_t)seq[j]]++; }
      std::set<int64_t> ready;
      for (size_t k = 0; k < el.size(); ++k) if (!indeg[k]) ready.insert((int64_t)k);
      while (!ready.empty()) {
        const int64_t k = *ready.begin();
        ready.erase(ready.begin());
        order.push_back(el[(size_t)k]);
        for (int64_t nx : succ[(size_t)k]) if (--indeg[(size_t)nx] == 0) ready.insert(nx);
      }
      if (order.size() != el.size()) return reject(e, FW_ERR_INVALID_ARG, "the windows' lists disagree on the arrival order");
    }
    for (int64_t n = wins.rbegin()->first; R == 1 && n >= wins.begin()->first; --n) {
      std::vector<size_t> T;   // the key's known elements of window n's newer slices, in arrival order
      for (size_t q = 0; q < order.size(); ++q)
        if (order[q].m > n && order[q].m < n + K) T.push_back(q);
      auto it = wins.find(n);
      if (it == wins.end()) {
        if (!T.empty()) return reject(e, FW_ERR_INVALID_ARG, "a window of the key is missing between its windows");
        continue;
      }
      std::vector<std::pair<size_t, El>> ins;   // (insert after this order index, or SIZE_MAX: at the front)
      size_t t = 0, pred = SIZE_MAX;
      for (const auto& x : lists[it->second]) {
        if (t < T.size() && order[T[t]].v == x[0] && order[T[t]].f1 == x[1]) { pred = T[t++]; continue; }
        ins.push_back({pred, El{x[0], x[1], n}});
      }
      if (t != T.size()) return reject(e, FW_ERR_INVALID_ARG, "the windows' lists of a key do not share their slices");
      std::vector<El> next;
      next.reserve(order.size() + ins.size());
      size_t k = 0;
      while (k < ins.size() && ins[k].first == SIZE_MAX) next.push_back(ins[k++].second);
      for (size_t q = 0; q < order.size(); ++q) {
        next.push_back(order[q]);
        while (k < ins.size() && ins[k].first == q) next.push_back(ins[k++].second);
      }
      order.swap(next);
    }
    for (const auto& w : wins) {   // every window's list rebuilt from the slices
      const auto& want = lists[w.second];
      size_t j = 0;
      for (const El& x : order) {
        if (x.m < w.first * R || x.m >= w.first * R + K) continue;
        if (j >= want.size() || want[j][0] != x.v || want[j][1] != x.f1)
          return reject(e, FW_ERR_UNSUPPORTED, "sliding-window lists with equal elements in an order no slice split gives");
        ++j;
      }
      if (j != want.size()) return reject(e, FW_ERR_UNSUPPORTED, "sliding-window lists with equal elements in an order no slice split gives");
    }
    for (const El& x : order) slices[{x.m, key}].push_back({e->restore_ord++, x.v, x.f1});
  }
  // the slices and keys into the directory and the slice table, then their elements into the slices' buffers
  std::vector<int64_t> ent;
  for (const auto& kv : slices) {
    const int64_t w[FW_SNAP_ENTRY_WORDS] = {kv.first.first, kv.first.second, 0, INT64_MAX, INT64_MIN, 0, kv.second[0][0], 0};
    ent.insert(ent.end(), w, w + FW_SNAP_ENTRY_WORDS);
  }
  int rc = restore_entries(e, wm, ent.data(), (int64_t)slices.size(), 0);
  if (rc) return rc;
  return append_list_elements(e, [&](auto add) {
    for (const auto& kv : slices)
      for (const auto& x : kv.second) add(kv.first.first, kv.first.second, x[0], x[1], x[2]);
  });
}

// PurgingTrigger + allowed lateness: a window purged by its fire keeps its keys' cleanup timers without state.  The
// timers beyond the ones the panes imply (`got` and `want` sorted) must all be such timers — of a window of the
// assigner (every `step` ms) in which the key holds no pane, and, where `pending` asks, ahead of the watermark;
// each goes to sink(window number, key, window start)
template <class Sink>
static int extra_cleanup_timers(fw_engine* e, int32_t kg, const std::vector<KgPane>& panes, const std::vector<fwkg::Timer>& got,
                                const std::vector<fwkg::Timer>& want, int64_t step, bool pending, int64_t watermark, Sink sink) {
  const fw_config& c = e->cfg;
  const char* differ = "timers differ from the ones the panes imply at the restore watermark";
  if (!std::includes(got.begin(), got.end(), want.begin(), want.end())) return reject(e, FW_ERR_UNSUPPORTED, differ);
  std::vector<fwkg::Timer> extra;
  std::set_difference(got.begin(), got.end(), want.begin(), want.end(), std::back_inserter(extra));
  std::set<std::pair<int64_t, int64_t>> has;
  for (const KgPane& p : panes) has.insert({p.start, p.key});
  for (const fwkg::Timer& t : extra) {
    const int64_t m = fw::floor_div(fw::jsub(t.start, c.offset), step);
    const int64_t max_ts = fw::jsub(t.end, 1), ct = fw::cleanup_time(max_ts, c.allowed_lateness);
    if (host_window_start(c, m) != t.start || t.end != fw::jadd(t.start, c.size) || t.ts != ct || ct == max_ts ||
        (pending && ct <= watermark) || has.count({t.start, t.key}) || host_key_group(e->s, t.key) != kg)
      return reject(e, FW_ERR_UNSUPPORTED, differ);
    sink(m, t.key, t.start);
  }
  return FW_OK;
}

static int window_restore_kg_flink(fw_engine* e, int32_t kg, const fw_state_layout* layout, int64_t watermark,
                                   const void* state, int64_t state_len, const void* timers, int64_t timers_len) {
  const fw_config& c = e->cfg;
  const fw::Spec& s = e->s;
  const bool sliding = c.assigner == FW_SLIDING;
  const bool sl_purge = sliding && c.trigger == FW_TRIGGER_PURGING_EVENT_TIME && c.allowed_lateness > 0;
  if (sl_purge && !s.first)
    return reject(e, FW_ERR_UNSUPPORTED, "sliding windows under PurgingTrigger with allowed lateness need first-arrival "
                                         "tracking (keep_first_f1)");
  if (sl_purge && e->adv_log.empty()) e->adv_log.push_back({watermark, 0});   // windows fired before: at the restore
  std::vector<KgPane> panes;
  std::vector<int64_t> slice_of;
  std::vector<std::vector<std::array<int64_t, 2>>> lists;   // list state: each entry's elements (value bits, f1)
  bool present = false;
  if (state_len > 0) {
    fwkg::BeIn in(state, state_len);
    if (in.i32() != kg) return reject(e, FW_ERR_INVALID_ARG, "state section of another key group");
    if (in.i16() != 0) return reject(e, FW_ERR_UNSUPPORTED, "keyed state other than window-contents");
    present = in.u8() != 0;
    std::set<std::pair<int64_t, int64_t>> seen;
    // tumbling: the window's slice; sliding: the window number (its own pane holds the window's state)
    const int64_t step = sliding ? c.slide : c.size;
    int64_t m = 0;
    int rc = FW_OK;
    const fwkg::WcFail f = !present ? fwkg::WcFail::none : fwkg::read_window_contents(
        in, wc_layout(e, layout),
        [&](int64_t start, int64_t end) {
          m = fw::floor_div(fw::jsub(start, c.offset), step);
          if (end != fw::jadd(start, c.size) || host_window_start(c, m) != start ||
              fw::window_start_with_offset(start, c.offset, step) != start)
            rc = reject(e, FW_ERR_INVALID_ARG, "namespace is not a window of this assigner");
          return rc == FW_OK;
        },
        [&](int64_t start, int64_t end, fwkg::WcEntry& ent) {
          KgPane p{start, end, ent.key, 0, INT64_MAX, INT64_MIN, 0, 0, 0, false};
          pane_from_words(e, layout, ent.word, p);
          if (e->list) lists.push_back(std::move(ent.el));
          if (s.fold) p = unfold_pane(e, p);
          if (host_key_group(s, p.key) != kg) rc = reject(e, FW_ERR_KEY_GROUP, "state entry key outside its key group");
          else if (!seen.insert({m, p.key}).second) rc = reject(e, FW_ERR_INVALID_ARG, "duplicate (window, key) entry");
          if (rc) return false;
          panes.push_back(p);
          slice_of.push_back(m);
          return true;
        });
    if (f == fwkg::WcFail::stopped) return rc;
    if (f != fwkg::WcFail::none) return reject_state(e, f);
    if (!in.done()) return reject(e, FW_ERR_INVALID_ARG, "state section truncated or with trailing bytes");
  }
  // timers: exactly the ones the panes imply at `watermark` (the engine's timers are implicit)
  std::vector<fwkg::Timer> got_in_order, want;
  if (int rc = read_timer_section(e, timers, timers_len, got_in_order)) return rc;
  std::vector<fwkg::Timer> got = got_in_order;
  // a window ahead of `watermark` whose panes carry no trigger timer fired before the checkpoint (the
  // reference restarts its timer service at Long.MIN_VALUE): it is restored disarmed — it fires again only for
  // keys a later record re-arms before the watermark passes it.  The panes of one window agree, in every key
  // group (an aligned checkpoint fired a window's timers for all its keys at one watermark)
  std::sort(got.begin(), got.end());
  std::set<int64_t> dis_now, armed_now;
  for (size_t i = 0; i < panes.size(); ++i) {
    const KgPane& p = panes[i];
    const int64_t max_ts = fw::jsub(p.end, 1), ct = fw::cleanup_time(max_ts, c.allowed_lateness);
    if (ct <= watermark) return reject(e, FW_ERR_UNSUPPORTED, "pane past its cleanup time at the restore watermark");
    if (max_ts <= watermark) continue;
    const bool has = std::binary_search(got.begin(), got.end(), fwkg::Timer{p.key, p.start, p.end, max_ts});
    (has ? armed_now : dis_now).insert(slice_of[i]);
  }
  for (int64_t m : dis_now)
    if (armed_now.count(m) || e->armed_windows.count(m) || c.allowed_lateness == 0)
      return reject(e, FW_ERR_UNSUPPORTED, "a window with and without trigger timers (not an aligned checkpoint)");
  for (int64_t m : armed_now)
    if (e->disarmed.count(m)) return reject(e, FW_ERR_UNSUPPORTED, "a window with and without trigger timers (not an aligned checkpoint)");
  for (size_t i = 0; i < panes.size(); ++i) {
    const KgPane& p = panes[i];
    const int64_t max_ts = fw::jsub(p.end, 1), ct = fw::cleanup_time(max_ts, c.allowed_lateness);
    if (max_ts > watermark && !dis_now.count(slice_of[i])) want.push_back({p.key, p.start, p.end, max_ts});
    if (ct != max_ts) want.push_back({p.key, p.start, p.end, ct});
  }
  std::sort(want.begin(), want.end());
  // PurgingTrigger + allowed lateness: a window purged by its fire keeps its keys' cleanup timers without state
  std::vector<int64_t> ghosts;   // restore entries (window, key, .., ordinal)
  if (s.gtag) {   // (tumbling: tracked per window like the purged windows of this run; only ones still pending)
    if (int rc = extra_cleanup_timers(e, kg, panes, got, want, c.size, true, watermark, [&](int64_t m, int64_t key, int64_t) {
          const int64_t w[FW_SNAP_ENTRY_WORDS] = {m, key, 0, 0, 0, 0, 0, 0};
          ghosts.insert(ghosts.end(), w, w + FW_SNAP_ENTRY_WORDS);
        }))
      return rc;
  } else if (sl_purge) {   // (sliding: of fired, purged windows, each key whose first element preceded the fire)
    if (int rc = extra_cleanup_timers(e, kg, panes, got, want, c.slide, false, watermark,
                                      [&](int64_t, int64_t key, int64_t start) { e->sl_ghost.insert({start, key}); }))
      return rc;
  } else if (got != want) {
    return reject(e, FW_ERR_UNSUPPORTED, "timers differ from the ones the panes imply at the restore watermark");
  }
  if (e->list && sliding && !dis_now.empty())
    return reject(e, FW_ERR_UNSUPPORTED, "sliding-window list state restored below a window that fired before the checkpoint");
  auto note_restored = [&] {   // the timers' blob order, and that the key group's table existed
    for (const auto& t : got_in_order) e->restored_timer_rank[t] = (int64_t)e->restored_timer_rank.size();
    if (e->kg_touched.empty()) e->kg_touched.assign((size_t)(s.kg_end - s.kg_start + 1), 0);
    if (present) e->kg_touched[(size_t)(kg - s.kg_start)] = 1;
  };
  if (e->list && sliding) {
    note_restored();
    return restore_sliding_lists(e, watermark, panes, slice_of, lists);
  }
  if (!dis_now.empty() && !e->s.disarm) {   // per-slot flags and per-pane re-arm marks, first needed here
    e->s.disarm = e->alloc<uint8_t>((size_t)s.P);
    e->s.armed = e->alloc<uint8_t>((size_t)s.P * (size_t)s.stride);
    if (int rc = upload_spec(e)) return rc;
    if (!e->s.disarm || !e->s.armed) return reject(e, FW_ERR_DEVICE, "out of device memory");
    HIPCHK(e, hipMemset(e->s.disarm, 0, (size_t)s.P));
    HIPCHK(e, hipMemset(e->s.armed, 0, (size_t)s.P * (size_t)s.stride));
  }
  for (int64_t m : dis_now) {
    e->disarmed.insert(m);
    const uint8_t one = 1;
    HIPCHK(e, hipMemcpy(e->s.disarm + floor_mod(m, s.P), &one, 1, hipMemcpyHostToDevice));
  }
  e->armed_windows.insert(armed_now.begin(), armed_now.end());
  // arrival ordinals in blob order: restored panes precede every later record, and keep the blob's
  // (HashMap iteration) order as their insertion order, as readStateTableForKeyGroup's puts do
  std::vector<int64_t> ent(panes.size() * FW_SNAP_ENTRY_WORDS);
  std::vector<int64_t> list_ord(panes.size());
  for (size_t i = 0; i < panes.size(); ++i) {
    const KgPane& p = panes[i];
    const int64_t ord = e->restore_ord;
    e->restore_ord += e->list ? (int64_t)lists[i].size() : 1;   // list state: one ordinal per element
    list_ord[i] = ord;
    const int64_t w[FW_SNAP_ENTRY_WORDS] = {slice_of[i], p.key, p.sum, p.mn, p.mx, s.by ? ord : p.cnt, ord, p.f1};
    memcpy(&ent[i * FW_SNAP_ENTRY_WORDS], w, sizeof(w));
  }
  note_restored();
  int rc = restore_entries(e, watermark, ent.data(), (int64_t)panes.size(), sliding ? 1 : 0);
  if (rc) return rc;
  if (e->list)   // (tumbling: each entry's elements into its slice, with their ordinals in blob order)
    return append_list_elements(e, [&](auto add) {
      for (size_t i = 0; i < panes.size(); ++i)
        for (size_t q = 0; q < lists[i].size(); ++q)
          add(slice_of[i], panes[i].key, list_ord[i] + (int64_t)q, lists[i][q][0], lists[i][q][1]);
    });
  if (!s.gtag) return rc;
  // windows within their lateness at the restore watermark (later per-element fires purge them again), and the
  // restored cleanup timers without state, each with its arrival ordinal (after the panes', in blob order)
  rc = ghost_advance(e, INT64_MIN, watermark);
  const int64_t ng = (int64_t)(ghosts.size() / FW_SNAP_ENTRY_WORDS);
  for (int64_t j = 0; j < ng && !rc; ++j) {
    ghosts[(size_t)j * FW_SNAP_ENTRY_WORDS + 6] = s.first ? e->restore_ord++ : 0;
    rc = ghost_track(e, ghosts[(size_t)j * FW_SNAP_ENTRY_WORDS]);
  }
  if (rc) return rc;
  return restore_entries(e, watermark, ghosts.data(), ng, 2);
}

extern "C" int fw_restore_kg_flink(fw_engine* e, int32_t kg, const fw_state_layout* layout, int64_t watermark,
                                   const void* state, int64_t state_len, const void* timers, int64_t timers_len) {
  if (!e || (!state && state_len) || !timers || state_len < 0) return FW_ERR_INVALID_ARG;
  if (e->sticky) return e->sticky;
  if (e->pushes > 0 || e->records_in > 0) return reject(e, FW_ERR_INVALID_ARG, "restore after the first push");
  if (kg < e->s.kg_start || kg > e->s.kg_end)
    return reject(e, FW_ERR_INVALID_ARG, "Key Group " + std::to_string(kg) + " does not belong to the local range.");
  // (the next two are both FW_ERR_INVALID_ARG, whichever comes first)
  if (e->restored && watermark != e->cur_wm) return reject(e, FW_ERR_INVALID_ARG, "key groups restored at different watermarks");
  if (int rc = check_state_layout(e, layout)) return rc;
  return (e->session ? session_restore_kg_flink : window_restore_kg_flink)(e, kg, layout, watermark, state, state_len,
                                                                           timers, timers_len);
}

