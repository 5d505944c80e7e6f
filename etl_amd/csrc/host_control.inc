// Part of host.cpp (included there, one translation unit): the control plane — schema slots and masks (schema.rs:99-129, 380-441), the wire reader of Relation / Message bodies, the serde-style JSON pull parser of DDL messages (codec/event.rs:37-106), handle_relation / handle_ddl (apply.rs:2160-2276, 2363-2440), the device slot table.

// ----------------------------------------------------------------- slots
int32_t make_slot(etlg_ctx* c, const SchemaPtr& sch, const std::vector<uint8_t>& repl, const std::vector<uint8_t>& ident) {
  auto s = std::make_unique<SlotHost>();
  uint32_t nid = 0;
  for (size_t i = 0; i < sch->cols.size(); i++) {
    if (repl[i] != 1) continue;
    etlg_slot_col sc{};
    sc.type_oid = sch->cols[i].type_oid;
    sc.stored_index = (uint16_t)i;
    sc.type_class = (uint8_t)type_class(sc.type_oid);
    sc.nullable = sch->cols[i].nullable;
    sc.identity = ident[i] == 1;
    sc.key_index = sc.identity ? (uint16_t)nid++ : (uint16_t)0xFFFF;
    s->cols.push_back(sc);
    s->pk.push_back(sch->cols[i].pk ? 1 : 0);
  }
  {  // identity type over the stored columns, as the reference infers it from the two masks
    bool has = false, m_pk = true, m_full = true;
    for (size_t i = 0; i < sch->cols.size(); i++) {
      const bool r = repl[i] == 1, id = ident[i] == 1;
      has |= id;
      if (id != (r && sch->cols[i].pk)) m_pk = false;
      if (id != r) m_full = false;
    }
    s->identity_type = !has ? 0 : m_pk ? 1 : m_full ? 2 : 3;
  }
  const uint32_t n = (uint32_t)s->cols.size();
  etlg_slot_desc& d = s->desc;
  d = etlg_slot_desc{};
  d.table_id = sch->table_id; d.n_stored = (uint32_t)sch->cols.size(); d.snapshot_lsn = sch->snapshot;
  d.n_cols = n; d.n_ident = nid;
  d.state_bytes_full = 4 * ((n + 15) / 16);
  d.state_bytes_key = 4 * ((nid + 15) / 16);
  uint32_t off = d.state_bytes_full, koff = d.state_bytes_key;
  for (auto& sc : s->cols) {
    const uint32_t sb = slot_bytes(sc.type_class);
    sc.off_full = (uint16_t)off; off += sb;
    if (sc.identity) { sc.off_key = (uint16_t)koff; koff += sb; }
  }
  d.row_bytes_full = off; d.row_bytes_key = koff;
  d.cols = s->cols.data();
  c->slots.push_back(std::move(s));
  c->cs.n_slots = c->slots.size();
  c->slots_dirty = true;
  return (int32_t)c->slots.size() - 1;
}

SchemaPtr get_at_or_before(const ControlState& cs, uint32_t table_id, uint64_t snap) {
  auto it = cs.store.find(table_id);  // store/schema/table.rs:61-71
  if (it == cs.store.end()) return nullptr;
  auto ub = it->second.upper_bound(snap);
  if (ub == it->second.begin()) return nullptr;
  --ub;
  return ub->second;
}

bool should_apply(const etlg_ctx* c, uint32_t table_id, uint64_t final_lsn) {  // apply.rs:2836-2867, 3514-3519
  if (c->worker == ETLG_WORKER_TABLE_SYNC) return c->sync_table == table_id;
  auto it = c->states.find(table_id);
  if (it == c->states.end()) return false;
  if (it->second.kind == ETLG_TS_READY) return true;
  if (it->second.kind == ETLG_TS_SYNC_DONE) return it->second.lsn <= final_lsn;
  return false;
}

// --------------------------------------------------------- tiny byte reader
struct Rd {
  const uint8_t* p; size_t n; size_t i = 0; bool ok = true;
  bool need(size_t k) { if (!ok || n - i < k) { ok = false; return false; } return true; }
  uint8_t u8() { return need(1) ? p[i++] : 0; }
  uint16_t u16() { if (!need(2)) return 0; uint16_t v = (uint16_t)(p[i] << 8 | p[i + 1]); i += 2; return v; }
  uint32_t u32() { if (!need(4)) return 0; uint32_t v = (uint32_t)p[i] << 24 | (uint32_t)p[i + 1] << 16 | (uint32_t)p[i + 2] << 8 | p[i + 3]; i += 4; return v; }
  uint64_t u64() { uint64_t h = u32(); return h << 32 | u32(); }
  std::string_view cstr() {
    if (!ok) return {};
    const void* z = memchr(p + i, 0, n - i);
    if (!z) { ok = false; return {}; }
    size_t len = (const uint8_t*)z - (p + i);
    std::string_view r((const char*)p + i, len);
    i += len + 1;
    return r;
  }
};

bool utf8_ok(std::string_view s) {  // String::from_utf8 in the cstr accessors
  const uint8_t* p = (const uint8_t*)s.data(); size_t n = s.size(), i = 0;
  while (i < n) {
    uint8_t c = p[i];
    if (c < 0x80) { i++; continue; }
    size_t need; uint8_t lo = 0x80, hi = 0xBF;
    if (c >= 0xC2 && c <= 0xDF) need = 1;
    else if (c >= 0xE0 && c <= 0xEF) { need = 2; if (c == 0xE0) lo = 0xA0; if (c == 0xED) hi = 0x9F; }
    else if (c >= 0xF0 && c <= 0xF4) { need = 3; if (c == 0xF0) lo = 0x90; if (c == 0xF4) hi = 0x8F; }
    else return false;
    if (n - i <= need) return false;
    if (p[i + 1] < lo || p[i + 1] > hi) return false;
    for (size_t k = 2; k <= need; k++) if ((p[i + k] & 0xC0) != 0x80) return false;
    i += need + 1;
  }
  return true;
}

// ------------------------------------------------- DDL message (JSON) reader
// SchemaChangeMessage (codec/event.rs:37-56, 96-106, 182-196) with serde's
// struct rules: unknown fields skipped, missing / duplicate / mistyped fields
// are errors, null only for Option. A pull parser: no DOM is built.
struct Json {
  const char* p; const char* e; int depth = 0; bool bad = false;
  void ws() { while (p < e && (*p == ' ' || *p == '\n' || *p == '\t' || *p == '\r')) p++; }
  bool eat(char c) { ws(); if (p < e && *p == c) { p++; return true; } return false; }
  bool peek(char c) { ws(); return p < e && *p == c; }
  bool fail() { bad = true; return false; }
  static void utf8_push(std::string& o, unsigned cp) {
    if (cp < 0x80) o += (char)cp;
    else if (cp < 0x800) { o += (char)(0xC0 | cp >> 6); o += (char)(0x80 | (cp & 63)); }
    else if (cp < 0x10000) { o += (char)(0xE0 | cp >> 12); o += (char)(0x80 | ((cp >> 6) & 63)); o += (char)(0x80 | (cp & 63)); }
    else { o += (char)(0xF0 | cp >> 18); o += (char)(0x80 | ((cp >> 12) & 63)); o += (char)(0x80 | ((cp >> 6) & 63)); o += (char)(0x80 | (cp & 63)); }
  }
  bool hex4(unsigned& v) {
    if (e - p < 4) return fail();
    v = 0;
    for (int k = 0; k < 4; k++) {
      char h = *p++; int d = h >= '0' && h <= '9' ? h - '0' : h >= 'a' && h <= 'f' ? h - 'a' + 10 : h >= 'A' && h <= 'F' ? h - 'A' + 10 : -1;
      if (d < 0) return fail();
      v = v * 16 + (unsigned)d;
    }
    return true;
  }
  bool string(std::string* out) {
    ws();
    if (p >= e || *p != '"') return fail();
    p++;
    while (p < e) {
      unsigned char c = (unsigned char)*p++;
      if (c == '"') return true;
      if (c < 0x20) return fail();
      if (c != '\\') { if (out) *out += (char)c; continue; }
      if (p >= e) return fail();
      char x = *p++;
      char plain = 0;
      switch (x) {
        case '"': plain = '"'; break; case '\\': plain = '\\'; break; case '/': plain = '/'; break;
        case 'b': plain = '\b'; break; case 'f': plain = '\f'; break; case 'n': plain = '\n'; break;
        case 'r': plain = '\r'; break; case 't': plain = '\t'; break;
        case 'u': {
          unsigned v;
          if (!hex4(v)) return false;
          if (v >= 0xDC00 && v <= 0xDFFF) return fail();
          if (v >= 0xD800 && v <= 0xDBFF) {
            if (e - p < 2 || p[0] != '\\' || p[1] != 'u') return fail();
            p += 2;
            unsigned w;
            if (!hex4(w)) return false;
            if (w < 0xDC00 || w > 0xDFFF) return fail();
            v = 0x10000 + ((v - 0xD800) << 10) + (w - 0xDC00);
          }
          if (out) utf8_push(*out, v);
          continue;
        }
        default: return fail();
      }
      if (out) *out += plain;
    }
    return fail();
  }
  // number literal -> integer in [lo, hi]; fractions / exponents are type errors
  bool integer(int64_t lo, uint64_t hi, int64_t& out) {
    ws();
    const char* s = p;
    bool neg = false;
    if (p < e && *p == '-') { neg = true; p++; }
    if (p >= e || *p < '0' || *p > '9') return fail();
    if (*p == '0') p++; else while (p < e && *p >= '0' && *p <= '9') p++;
    if (p < e && (*p == '.' || *p == 'e' || *p == 'E')) return fail();
    unsigned __int128 mag = 0;
    for (const char* q = s + (neg ? 1 : 0); q < p; q++) { mag = mag * 10 + (unsigned)(*q - '0'); if (mag > ((unsigned __int128)1 << 70)) return fail(); }
    if (neg) { if (mag > (unsigned __int128)(-(lo + 1)) + 1) return fail(); out = (int64_t)(-(__int128)mag); }
    else { if (mag > hi) return fail(); out = (int64_t)(uint64_t)mag; }
    return true;
  }
  bool skip_number() {
    if (p < e && *p == '-') p++;
    if (p >= e) return fail();
    if (*p == '0') p++;
    else if (*p >= '1' && *p <= '9') while (p < e && *p >= '0' && *p <= '9') p++;
    else return fail();
    if (p < e && *p == '.') { p++; if (p >= e || *p < '0' || *p > '9') return fail(); while (p < e && *p >= '0' && *p <= '9') p++; }
    if (p < e && (*p == 'e' || *p == 'E')) { p++; if (p < e && (*p == '+' || *p == '-')) p++; if (p >= e || *p < '0' || *p > '9') return fail(); while (p < e && *p >= '0' && *p <= '9') p++; }
    return true;
  }
  bool lit(const char* s) { size_t n = strlen(s); if ((size_t)(e - p) < n || memcmp(p, s, n)) return fail(); p += n; return true; }
  bool skip_value() {
    ws();
    if (p >= e) return fail();
    switch (*p) {
      case '{': {
        if (++depth > 128) return fail();
        p++;
        if (eat('}')) { depth--; return true; }
        for (;;) {
          if (!string(nullptr) || !eat(':') || !skip_value()) return fail();
          if (eat(',')) continue;
          if (eat('}')) { depth--; return true; }
          return fail();
        }
      }
      case '[': {
        if (++depth > 128) return fail();
        p++;
        if (eat(']')) { depth--; return true; }
        for (;;) {
          if (!skip_value()) return false;
          if (eat(',')) continue;
          if (eat(']')) { depth--; return true; }
          return fail();
        }
      }
      case '"': return string(nullptr);
      case 't': return lit("true");
      case 'f': return lit("false");
      case 'n': return lit("null");
      default: return skip_number();
    }
  }
  // iterate an object: calls f(key) for each member; f must consume the value
  template <class F>
  bool object(F f) {
    if (!eat('{')) return fail();
    if (++depth > 128) return fail();
    if (eat('}')) { depth--; return true; }
    for (;;) {
      std::string key;
      if (!string(&key) || !eat(':')) return fail();
      if (!f(key)) return fail();
      if (eat(',')) continue;
      if (eat('}')) { depth--; return true; }
      return fail();
    }
  }
  template <class F>
  bool array(F f) {
    if (!eat('[')) return fail();
    if (++depth > 128) return fail();
    if (eat(']')) { depth--; return true; }
    for (;;) {
      if (!f()) return fail();
      if (eat(',')) continue;
      if (eat(']')) { depth--; return true; }
      return fail();
    }
  }
  bool boolean(bool& b) { ws(); if (p < e && *p == 't') { b = true; return lit("true"); } if (p < e && *p == 'f') { b = false; return lit("false"); } return fail(); }
};

bool parse_ddl(std::string_view content, uint64_t snapshot, std::shared_ptr<StoredSchema>& out) {
  Json j{content.data(), content.data() + content.size()};
  auto sch = std::make_shared<StoredSchema>();
  sch->snapshot = snapshot;
  int seen_tag = 0, seen_nsp = 0, seen_rel = 0, seen_oid = 0, seen_ident = 0, seen_cols = 0;
  std::vector<int32_t> pks;
  bool ok = j.object([&](const std::string& k) {
    if (k == "command_tag") { seen_tag++; return j.string(nullptr); }
    if (k == "nspname") { seen_nsp++; return j.string(&sch->nsp); }
    if (k == "relname") { seen_rel++; return j.string(&sch->name); }
    if (k == "oid") { seen_oid++; int64_t v; if (!j.integer(INT64_MIN, INT64_MAX, v)) return false; sch->table_id = (uint32_t)v; return true; }
    if (k == "identity") {
      seen_ident++;
      int s_pk = 0, s_rid = 0, s_rix = 0;
      bool o = j.object([&](const std::string& k2) {
        if (k2 == "primary_key_attnums") { s_pk++; return j.array([&] { int64_t v; if (!j.integer(INT32_MIN, INT32_MAX, v)) return false; pks.push_back((int32_t)v); return true; }); }
        if (k2 == "relreplident") { s_rid++; return j.string(nullptr); }
        if (k2 == "replica_identity_index_attnums") { s_rix++; return j.array([&] { int64_t v; return j.integer(INT32_MIN, INT32_MAX, v); }); }
        return j.skip_value();
      });
      return o && s_pk == 1 && s_rid == 1 && s_rix == 1;
    }
    if (k == "columns") {
      seen_cols++;
      return j.array([&] {
        StoredCol c{};
        int s_n = 0, s_t = 0, s_m = 0, s_a = 0, s_nn = 0, s_d = 0;
        bool notnull = false;
        bool o = j.object([&](const std::string& k2) {
          int64_t v;
          if (k2 == "attname") { s_n++; return j.string(&c.name); }
          if (k2 == "atttypid") { s_t++; if (!j.integer(0, UINT32_MAX, v)) return false; c.type_oid = (uint32_t)v; return true; }
          if (k2 == "atttypmod") { s_m++; if (!j.integer(INT32_MIN, INT32_MAX, v)) return false; c.typmod = (int32_t)v; return true; }
          if (k2 == "attnum") { s_a++; if (!j.integer(INT32_MIN, INT32_MAX, v)) return false; c.attnum = (int32_t)v; return true; }
          if (k2 == "attnotnull") { s_nn++; return j.boolean(notnull); }
          if (k2 == "default_expression") { s_d++; if (j.peek('n')) return j.lit("null"); return j.string(nullptr); }
          return j.skip_value();
        });
        if (!o || s_n != 1 || s_t != 1 || s_m != 1 || s_a != 1 || s_nn != 1 || s_d > 1) return false;
        c.nullable = !notnull;
        sch->cols.push_back(std::move(c));
        return true;
      });
    }
    return j.skip_value();
  });
  if (!ok || j.bad) return false;
  j.ws();
  if (j.p != j.e) return false;
  if (seen_tag != 1 || seen_nsp != 1 || seen_rel != 1 || seen_oid != 1 || seen_ident != 1 || seen_cols != 1) return false;
  for (auto& c : sch->cols) c.pk = std::find(pks.begin(), pks.end(), c.attnum) != pks.end();
  std::stable_sort(sch->cols.begin(), sch->cols.end(), [](const StoredCol& a, const StoredCol& b) { return a.attnum < b.attnum; });
  out = std::move(sch);
  return true;
}

// ----------------------------------------------------- control-plane frames

// handle_relation_message (apply.rs:2363-2440) for one R frame.
HostErr handle_relation(etlg_ctx* c, const CtrlFrame& cf, const uint8_t* body, size_t n, std::vector<EpochRec>& eps) {
  Rd r{body, n};
  const uint32_t rel_id = r.u32();
  (void)r.cstr(); (void)r.cstr();
  const uint8_t replident = r.u8();
  if (!r.ok || (replident != 'd' && replident != 'n' && replident != 'f' && replident != 'i')) return {ETLG_E_WIRE, RK_WIRE};
  const int16_t nc = (int16_t)r.u16();
  if (!r.ok || nc < 0) return {ETLG_E_WIRE, RK_WIRE};
  struct RC { int8_t flags; std::string_view name; };
  std::vector<RC> rcs;
  for (int k = 0; k < nc; k++) {
    RC x; x.flags = (int8_t)r.u8(); x.name = r.cstr(); (void)r.u32(); (void)r.u32();
    if (!r.ok) return {ETLG_E_WIRE, RK_WIRE};
    rcs.push_back(x);
  }
  if (!cf.in_txn) return {ETLG_E_TXN_STATE, RK_TXN};
  if (!should_apply(c, rel_id, cf.final_lsn)) return {};
  // parse_replicated_column_names / parse_replica_identity_column_names (codec/event.rs:352-396)
  std::set<std::string> repl, ident;
  for (auto& x : rcs) { if (!utf8_ok(x.name)) return {ETLG_E_IO, RK_SCHEMA}; repl.emplace(x.name); }
  for (auto& x : rcs) if (replident == 'f' || (x.flags & 1) == 1) ident.emplace(x.name);
  auto cit = c->cs.cache.find(rel_id);
  const bool used_bootstrap = cit == c->cs.cache.end();
  const uint64_t snap = used_bootstrap ? c->bootstrap : cit->second.snapshot;
  SchemaPtr sch = get_at_or_before(c->cs, rel_id, snap);  // get_table_schema_for_relation, apply.rs:3643-3697
  if (!sch) return {ETLG_E_SCHEMA_NOT_FOUND, RK_SCHEMA};
  if (used_bootstrap) { if (sch->snapshot > snap) return {ETLG_E_BOOTSTRAP_SNAPSHOT, RK_SCHEMA}; }
  else if (sch->snapshot != snap) return {ETLG_E_SNAPSHOT_MISMATCH, RK_SCHEMA};
  // ReplicationMask::try_build / IdentityMask::try_build (schema.rs:30-61, 99-129, 220-227)
  std::set<std::string_view> have;
  for (auto& sc : sch->cols) have.insert(sc.name);
  for (auto& nme : repl) if (!have.count(nme)) return {ETLG_E_UNKNOWN_COLUMNS, RK_SCHEMA};
  for (auto& nme : ident) if (!have.count(nme)) return {ETLG_E_UNKNOWN_COLUMNS, RK_SCHEMA};
  std::vector<uint8_t> rm, im;
  for (auto& sc : sch->cols) { rm.push_back(repl.count(sc.name) ? 1 : 0); im.push_back(ident.count(sc.name) ? 1 : 0); }
  const int32_t slot = make_slot(c, sch, rm, im);
  c->cs.cache[rel_id] = CacheEntry{2, sch->snapshot, slot};  // note_ready
  c->side_dirty = true;
  eps.push_back({rel_id, DevEpoch{cf.frame, 2, slot, 1}});
  return {};
}

// handle_message (apply.rs:2160-2276) for one M frame; `wal_start` = snapshot id.
HostErr handle_ddl(etlg_ctx* c, const CtrlFrame& cf, uint64_t wal_start, const uint8_t* body, size_t n, std::vector<EpochRec>& eps) {
  Rd r{body, n};
  (void)r.u8(); (void)r.u64();
  std::string_view prefix = r.cstr();
  const int32_t len = (int32_t)r.u32();
  if (!r.ok || len < 0 || !r.need((size_t)len)) return {ETLG_E_WIRE, RK_WIRE};
  std::string_view content((const char*)body + r.i, (size_t)len);
  if (!utf8_ok(prefix)) return {ETLG_E_IO, RK_SCHEMA};
  if (prefix != "supabase_etl_ddl") return {};  // codec/event.rs:28
  if (!cf.in_txn) return {ETLG_E_TXN_STATE, RK_TXN};
  if (!utf8_ok(content)) return {ETLG_E_IO, RK_SCHEMA};
  std::shared_ptr<StoredSchema> sch;
  if (!parse_ddl(content, wal_start, sch)) return {ETLG_E_DDL_PARSE, RK_SCHEMA};
  if (!should_apply(c, sch->table_id, cf.final_lsn)) return {};
  const uint32_t tid = sch->table_id;
  c->cs.store[tid][sch->snapshot] = sch;                       // store_table_schema
  c->cs.cache[tid] = CacheEntry{1, wal_start, -1};             // note_waiting_for_relation
  c->side_dirty = true;
  eps.push_back({tid, DevEpoch{cf.frame, 1, -1, 0}});
  return {};
}

// The schema slots as the kernels read them. Slot ids are stable for the life of the context (the arenas name them), but a stream
// that changes schemas often leaves most of them dead: the device table holds only the slots in `live` (what the table cache, this
// batch's epochs or a table copy can reach), addressed by their position in it (DevSlot.host_id names the arena's id). The side
// tables then stay small enough for the LDS copy the single-pass kernels want (k_cells needs it) after thousands of DDL messages.
void build_slots(etlg_ctx* c, const std::vector<int32_t>& live, std::vector<DevSlot>& ds, std::vector<DevCol>& dc) {
  for (int32_t li : live) {   // ascending host ids: the device index of a slot is its position in `live`
    if (li < 0 || (size_t)li >= c->slots.size()) { DevSlot dead{}; dead.cols_base = (uint32_t)dc.size(); dead.host_id = (uint32_t)li; ds.push_back(dead); continue; }
    auto& s = c->slots[(size_t)li];
    DevSlot d{};
    d.host_id = (uint32_t)li;
    d.n_cols = s->desc.n_cols; d.n_ident = s->desc.n_ident; d.row_full = s->desc.row_bytes_full; d.row_key = s->desc.row_bytes_key;
    d.st_full = s->desc.state_bytes_full; d.st_key = s->desc.state_bytes_key; d.cols_base = (uint32_t)dc.size();
    {  // which columns can reach the heap, and for which of them the byte count depends on the text (DevSlot.has_var)
      const bool narrow = s->cols.size() <= 16;
      uint32_t ci = 0;
      for (auto& sc : s->cols) {
        const int32_t k = sc.type_class;
        // fixed-width classes never reach the heap — the temporal ones included: their rare non-ISO shapes are decoded on the device too
        // (chrono_fallback, values.hip.h). A float reaches it only as a DEFERRED text; numeric / bytea entries are sized from the text
        const bool heap = !(k == ETLG_TC_BOOL || k == ETLG_TC_I16 || k == ETLG_TC_I32 || k == ETLG_TC_I64 || k == ETLG_TC_U32 || k == ETLG_TC_UUID ||
                            k == ETLG_TC_DATE || k == ETLG_TC_TIME || k == ETLG_TC_TIMETZ || k == ETLG_TC_TIMESTAMP || k == ETLG_TC_TIMESTAMPTZ);
        const bool scan = heap && !(k == ETLG_TC_STRING || k == ETLG_TC_JSON || k == ETLG_TC_ARRAY);
        if (!narrow) { if (heap) d.has_var = 0xFFFFFFFFu; }
        else {
          if (heap) d.has_var |= 1u << ci;
          if (scan) d.has_var |= 1u << (16 + ci);
          if (sc.identity) {
            d.ident_mask |= 1u << ci;
            if (sc.key_index < 16) { if (heap) d.key_masks |= 1u << sc.key_index; if (scan) d.key_masks |= 1u << (16 + sc.key_index); }
          }
        }
        ci++;
      }
    }
    {  // (k_rows) heap ranks and the inverse of key_index
      const size_t base = dc.size();
      auto heap_class = [](int32_t k) {
        return !(k == ETLG_TC_BOOL || k == ETLG_TC_I16 || k == ETLG_TC_I32 || k == ETLG_TC_I64 || k == ETLG_TC_U32 || k == ETLG_TC_UUID ||
                 k == ETLG_TC_DATE || k == ETLG_TC_TIME || k == ETLG_TC_TIMETZ || k == ETLG_TC_TIMESTAMP || k == ETLG_TC_TIMESTAMPTZ);
      };
      uint32_t hf = 0;
      for (auto& sc : s->cols) {
        DevCol x{};
        x.cls = sc.type_class; x.nullable = sc.nullable; x.identity = sc.identity; x.off_full = sc.off_full; x.off_key = sc.off_key; x.key_index = sc.key_index;
        x.hr = 0xFFFFu;
        if (heap_class(sc.type_class)) { x.hr = (uint16_t)(0xFF00u | std::min<uint32_t>(hf, 0xFFu)); hf++; }
        dc.push_back(x);
      }
      // key layout: identity columns in key_index order
      const size_t n = s->cols.size();
      std::vector<int32_t> by_key(n, -1);
      for (size_t i = 0; i < n; i++) if (s->cols[i].identity && s->cols[i].key_index < n) by_key[s->cols[i].key_index] = (int32_t)i;
      uint32_t hk = 0;
      for (size_t j = 0; j < n; j++) {
        dc[base + j].key_col = by_key[j] >= 0 ? (uint8_t)std::min<int32_t>(by_key[j], 255) : (uint8_t)255;
        if (by_key[j] >= 0 && heap_class(s->cols[(size_t)by_key[j]].type_class)) {
          DevCol& x = dc[base + (size_t)by_key[j]];
          x.hr = (uint16_t)((x.hr & 0x00FFu) | (std::min<uint32_t>(hk, 0xFFu) << 8)); hk++;
        }
      }
    }
    ds.push_back(d);
  }
}

