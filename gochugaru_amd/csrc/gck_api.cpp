// gck_api.cpp — the extern "C" boundary (include/gck.h). Every entry point converts C++
// exceptions into a negative status plus a thread-local message (gck_last_error).
#include <pthread.h>
#include <sched.h>

#include <algorithm>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <string_view>
#include <thread>

#include "engine.hpp"
#include "slot_pack.hpp"
#include "select_plane.hpp"

namespace gck {

thread_local std::string g_last_error;

#define REQUIRE(cond, code, msg) \
  do {                           \
    if (!(cond)) throw Error(code, msg); \
  } while (0)

Engine::~Engine() {
  device_free(*this);
  host_free_all(*this);
}

void reset_caveats(Engine& e) {
  ++e.shape_gen;  // (with the schema and a snapshot file: the interner starts over too)
  e.caveat_instances.assign(1, {"", ""});
  e.caveat_ids.clear();
  e.caveat_expr.assign(1, nullptr);
  e.caveat_ctx.assign(1, cel::Object{});
  e.caveat_static.assign(1, (uint8_t)cel::TRUE);  // instance 0: no caveat
  e.caveat_row.assign(1, kNone);
  e.caveat_partial.clear();
}

// A caveat name + stored context (rel.Relationship.CaveatName/CaveatContext,
// rel/relationship.go:93-120). Identical pairs share one instance. The stored context is parsed
// and the expression evaluated over it alone once, here: a caveat it decides is a plain or an
// absent edge for every check; one left PARTIAL gets a row of the per-call outcome table.
uint32_t add_caveat_instance(Engine& e, const std::string& name, const std::string& json) {
  auto cd = e.schema->caveats.find(name);
  if (cd == e.schema->caveats.end()) throw Error(GCK_E_INVALID_ARGUMENT, "unknown caveat '" + name + "'");
  std::string key = name;
  key += '\0';
  key += json;
  auto hit = e.caveat_ids.find(key);
  if (hit != e.caveat_ids.end()) return hit->second;
  REQUIRE(e.caveat_instances.size() < 0xFFFFFFF0u, GCK_E_CAPACITY, "too many caveat instances");
  cel::Object ctx = cel::parse_context(json);
  const cel::Outcome o = cel::evaluate(*cd->second.expr, &ctx, nullptr);
  const uint32_t id = (uint32_t)e.caveat_instances.size();
  e.caveat_instances.emplace_back(name, json);
  e.caveat_expr.push_back(cd->second.expr);
  e.caveat_ctx.push_back(std::move(ctx));
  e.caveat_static.push_back((uint8_t)o);
  e.caveat_row.push_back(o == cel::PARTIAL ? (uint32_t)e.caveat_partial.size() : kNone);
  if (o == cel::PARTIAL) e.caveat_partial.push_back(id);
  e.caveat_ids.emplace(std::move(key), id);
  return id;
}

// The check-time caveat contexts of one call (engine.hpp CavCall). Each partial instance r
// (caveat_partial[r]) under context slot k + 1 (CheckBulkPermissionsRequestItem.Context,
// client/client.go:257) is evaluated with the instance's stored context taking precedence.
// While instances x contexts is small every pair is evaluated here into a dense table (identical
// context texts share their evaluations); beyond that the contexts are only copied, and the pairs
// a walk touches are parsed and evaluated on demand (engine.hip caveat_passes). An evaluation
// error is outcome 3: it fails only the checks whose walk meets it (GCK_ITEM_ERR_CAVEAT_EVAL).
constexpr size_t kDensePairs = 4096;  // evaluations done eagerly

static CavCall caveat_call(Engine& e, const char* const* ctxs, const size_t* lens, size_t n_ctx) {
  CavCall c;
  c.n_given = (uint32_t)std::min<size_t>(n_ctx, 0xFFFFFFFFu);
  const size_t rows = e.caveat_partial.size();
  if (n_ctx == 0 || rows == 0) return c;
  REQUIRE(n_ctx < (1ull << 31), GCK_E_INVALID_ARGUMENT, "too many check contexts");
  c.n_ctx = (uint32_t)n_ctx;
  if (!(e.cfg.flags & GCK_FLAG_LAZY_CAVEATS) && rows <= kDensePairs) {
    std::unordered_map<std::string_view, uint32_t> seen;
    seen.reserve(std::min<size_t>(n_ctx, 4 * kDensePairs));
    std::vector<std::string_view> dist;
    c.of_slot.resize(n_ctx);
    for (size_t k = 0; k < n_ctx && rows * dist.size() <= kDensePairs; ++k) {
      const std::string_view js(ctxs[k] ? ctxs[k] : "", ctxs[k] ? lens[k] : 0);
      auto it = seen.emplace(js, (uint32_t)dist.size()).first;
      if (it->second == dist.size()) dist.push_back(js);
      c.of_slot[k] = it->second;
    }
    if (rows * dist.size() <= kDensePairs) {
      const size_t nd = dist.size();
      c.n_dist = (uint32_t)nd;
      c.dense.resize(rows * nd);
      for (size_t k = 0; k < nd; ++k) {
        const cel::Object ctx = cel::parse_context(std::string(dist[k]));  // a malformed context fails the call
        for (size_t r = 0; r < rows; ++r) {
          const uint32_t id = e.caveat_partial[r];
          try {
            c.dense[r * nd + k] = (uint8_t)cel::evaluate(*e.caveat_expr[id], &e.caveat_ctx[id], &ctx);
          } catch (const Error&) {
            c.dense[r * nd + k] = 3;
          }
        }
      }
      return c;
    }
    c.of_slot.clear();
  }
  // lazy: one copy of the texts (a context is parsed when a walk first needs it; a malformed one
  // then fails the call)
  size_t total = 0;
  for (size_t k = 0; k < n_ctx; ++k) total += ctxs[k] ? lens[k] : 0;
  REQUIRE(total < (1ull << 32), GCK_E_INVALID_ARGUMENT, "check contexts above 4 GiB");
  auto text = std::make_shared<std::string>();
  auto off = std::make_shared<std::vector<uint32_t>>(n_ctx + 1);
  text->reserve(total);
  for (size_t k = 0; k < n_ctx; ++k) {
    (*off)[k] = (uint32_t)text->size();
    if (ctxs[k]) text->append(ctxs[k], lens[k]);
  }
  (*off)[n_ctx] = (uint32_t)text->size();
  c.text = std::move(text);
  c.off = std::move(off);
  return c;
}

void stage_tuple(Engine& e, const gck_tuple& t);
void stage_tuples(Engine& e, const gck_tuple* t, size_t n);

}  // namespace gck

using namespace gck;

// Watch batches staged ahead of their apply (gck_watch_stage): an engine-owned thread validates
// and groups batch k + 1 while batch k applies — a Watch consumer (client/client.go:370-413)
// receives the next batch while it applies the previous one. Each staged batch has its own
// grouping buffers; kSlots may be staged at once. The stager reads the schema and the interner
// under the engine lock held shared and briefly (group_updates' schema_mu), and records the
// engine's shape generation: a batch staged before a write that moved it is regrouped at apply.
struct WatchStager {
  static constexpr int kSlots = 4;
  struct Slot {
    const gck_update* ups = nullptr;
    size_t n = 0;
    uint64_t ticket = 0;  // 0: free
    int state = 0;        // 1 queued, 3 being grouped, 2 grouped (or failed)
    bool ok = false;
    uint64_t gen = 0;
    std::vector<gck_update> mine;  // (a partitioned rank's own updates)
    GroupBuffers buf;
    const std::vector<UpdateGroup>* groups = nullptr;
  } slots[kSlots];
  std::mutex m;
  std::condition_variable cv_job, cv_done;
  // two threads: a consumer holding the next two responses has both grouped beside its apply (the
  // grouping of one config-5 batch takes about as long as an apply, ~80-100 us)
  static constexpr int kThreads = 2;
  std::thread th[kThreads];
  bool stop = false;
  uint64_t next_ticket = 1;
  ~WatchStager() {
    {
      std::lock_guard<std::mutex> g(m);
      stop = true;
    }
    cv_job.notify_all();
    for (std::thread& t : th)
      if (t.joinable()) t.join();
  }
};

struct gck_engine {
  Engine impl;
  WatchStager stage;  // (destroyed first: its thread ends before the engine does)
};

template <class F>
static int guard(F&& f) {
  try {
    f();  // (a success leaves the message of the thread's last failure, as errno: a caller's loop that
          // drains its batches after an error still reads that error's message)
    return GCK_OK;
  } catch (const Error& ex) {
    g_last_error = ex.what();
    return ex.code;
  } catch (const std::bad_alloc&) {
    g_last_error = "host out of memory";
    return GCK_E_CAPACITY;
  } catch (const std::exception& ex) {
    g_last_error = ex.what();
    return GCK_E_INVALID_ARGUMENT;
  }
}

static Engine& need(gck_engine* e) {
  REQUIRE(e, GCK_E_INVALID_ARGUMENT, "null engine");
  return e->impl;
}

static Schema& need_schema(Engine& e) {
  REQUIRE(e.schema, GCK_E_STATE, "no schema loaded (gck_load_schema)");
  return *e.schema;
}

extern "C" {

// What changes the engine's state — schema, snapshot, Watch batches, caveat instances, partition
// — is serialised by Engine::writer_mu and holds the engine lock exclusively; a Watch batch takes
// the exclusive lock only to start and to publish its snapshot (apply_updates).
struct WriterLock {
  std::lock_guard<std::mutex> w;
  std::unique_lock<std::shared_mutex> lk;
  explicit WriterLock(Engine& e) : w(e.writer_mu), lk(e.mu) {}
};

static_assert(sizeof(gck_config) == 88, "gck_config layout (include/gck.h) changed: bump GCK_ABI_VERSION");
static_assert(sizeof(gck_stats) == 240, "gck_stats layout (include/gck.h) changed: bump GCK_ABI_VERSION");
static_assert(sizeof(gck_item) == 20 && sizeof(gck_tuple) == 32 && sizeof(gck_update) == 40, "item/tuple/update layout");

int gck_abi_version(void) { return GCK_ABI_VERSION; }

const char* gck_last_error(void) { return g_last_error.c_str(); }

int gck_create(const gck_config* cfg, gck_engine** out) {
  return guard([&] {
    REQUIRE(out, GCK_E_INVALID_ARGUMENT, "null out pointer");
    *out = nullptr;
    auto* e = new gck_engine();
    if (cfg) e->impl.cfg = *cfg;
    if (e->impl.cfg.device < 0) {
      delete e;
      throw Error(GCK_E_INVALID_ARGUMENT, "bad device ordinal");
    }
    if (e->impl.cfg.max_depth > 250) {  // frontier entries hold the depth in 8 bits
      delete e;
      throw Error(GCK_E_INVALID_ARGUMENT, "max_depth above 250");
    }
    reset_caveats(e->impl);
    *out = e;
  });
}

void gck_destroy(gck_engine* e) { delete e; }

int gck_load_schema(gck_engine* ge, const char* text, size_t len) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(text || !len, GCK_E_INVALID_ARGUMENT, "null schema text");
    auto sc = compile_schema(std::string(text ? text : "", len));
    WriterLock lk(e);
    drain_batches(e);
    e.schema = std::move(sc);
    partition_rules(e);
    e.schema_text.assign(text ? text : "", len);
    e.interner.assign(e.schema->types.size(), TypeInterner());
    reset_caveats(e);
    e.staged.clear();
    e.prebuilt.clear();
    e.staging = false;
    e.committed = false;
    device_free(e);
  });
}

int gck_type_id(gck_engine* ge, const char* name, size_t len, uint16_t* out) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(out && (name || !len), GCK_E_INVALID_ARGUMENT, "null argument");
    int t = need_schema(e).find_type(std::string(name, len));
    REQUIRE(t >= 0, GCK_E_NOT_FOUND, "unknown type '" + std::string(name, len) + "'");
    *out = (uint16_t)t;
  });
}

int gck_relation_id(gck_engine* ge, uint16_t type, const char* name, size_t len, uint16_t* out) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(out && (name || !len), GCK_E_INVALID_ARGUMENT, "null argument");
    int r = need_schema(e).find_rel(type, std::string(name, len));
    REQUIRE(r >= 0, GCK_E_NOT_FOUND, "unknown relation '" + std::string(name, len) + "'");
    *out = (uint16_t)r;
  });
}

int gck_type_count(gck_engine* ge, uint32_t* out) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(out, GCK_E_INVALID_ARGUMENT, "null out");
    *out = (uint32_t)need_schema(e).types.size();
  });
}

int gck_relation_count(gck_engine* ge, uint32_t* out) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(out, GCK_E_INVALID_ARGUMENT, "null out");
    *out = (uint32_t)need_schema(e).rels.size();
  });
}

int gck_intern(gck_engine* ge, uint16_t type, const char* const* ids, const uint32_t* lens, size_t n,
               uint32_t flags, uint32_t* out_ids) {
  return guard([&] {
    Engine& e = need(ge);
    Schema& sc = need_schema(e);
    REQUIRE(type < sc.types.size(), GCK_E_INVALID_ARGUMENT, "unknown type id");
    REQUIRE(n == 0 || (ids && lens && out_ids), GCK_E_INVALID_ARGUMENT, "null argument");
    const bool create = flags & GCK_INTERN_CREATE;
    // creating ids is a write of the interner: it takes the writer lock as every writer does, so
    // that no Watch batch is between its interner mark and its rollback meanwhile (a text batch
    // that fails truncates the interner to the counts it recorded, gck_apply_updates_text)
    std::unique_lock<std::mutex> wlk(e.writer_mu, std::defer_lock);
    std::unique_lock<std::shared_mutex> lk(e.mu, std::defer_lock);
    std::shared_lock<std::shared_mutex> slk(e.mu, std::defer_lock);
    if (create) {
      wlk.lock();
      lk.lock();
    } else {
      slk.lock();
    }
    TypeInterner& ti = e.interner[type];
    std::string key;
    for (size_t i = 0; i < n; ++i) {
      key.assign(ids[i], lens[i]);
      if (key == "*") {
        out_ids[i] = GCK_ID_WILDCARD;
        continue;
      }
      auto it = ti.ids.find(key);
      if (it != ti.ids.end()) {
        out_ids[i] = it->second;
      } else if (create) {
        // (a partitioned graph: only a name's owner gives it an id, gck_part_intern_with)
        REQUIRE(e.part_world <= 1, GCK_E_STATE, "a partitioned engine interns a new name through its owner rank "
                                                "(gck_part_intern_with): '" + key + "'");
        REQUIRE(ti.count < GCK_ID_ABSENT, GCK_E_CAPACITY, "too many objects of one type");
        uint32_t id = ti.count++;
        ti.ids.emplace(key, id);
        if (ti.names.size() < ti.count) ti.names.resize(ti.count);
        ti.names[id] = key;
        out_ids[i] = id;
      } else {
        out_ids[i] = GCK_ID_ABSENT;
      }
    }
  });
}

int gck_object_count(gck_engine* ge, uint16_t type, uint32_t* out) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(type < need_schema(e).types.size() && out, GCK_E_INVALID_ARGUMENT, "bad argument");
    *out = e.interner[type].count;
  });
}

int gck_reserve_objects(gck_engine* ge, uint16_t type, uint32_t n) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(type < need_schema(e).types.size(), GCK_E_INVALID_ARGUMENT, "bad type");
    REQUIRE(n < GCK_ID_ABSENT, GCK_E_CAPACITY, "too many objects");
    WriterLock lk(e);
    TypeInterner& ti = e.interner[type];
    if (n > ti.count) ti.count = n;
  });
}

int gck_object_name(gck_engine* ge, uint16_t type, uint32_t id, char* buf, size_t cap, size_t* out_len) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(type < need_schema(e).types.size(), GCK_E_INVALID_ARGUMENT, "bad type");
    TypeInterner& ti = e.interner[type];
    REQUIRE(id < ti.count, GCK_E_NOT_FOUND, "unknown object id");
    auto rv = ti.rev.find(id);
    std::string nm = id < ti.names.size() && !ti.names[id].empty() ? ti.names[id]
                     : rv != ti.rev.end()                           ? rv->second
                                                                    : std::to_string(id);
    if (out_len) *out_len = nm.size();
    if (buf && cap) {
      size_t k = std::min(cap - 1, nm.size());
      std::memcpy(buf, nm.data(), k);
      buf[k] = 0;
    }
  });
}

int gck_add_caveat_instance(gck_engine* ge, const char* name, size_t name_len, const char* json,
                            size_t json_len, uint32_t* out_id) {
  return guard([&] {
    Engine& e = need(ge);
    need_schema(e);
    REQUIRE(name && out_id, GCK_E_INVALID_ARGUMENT, "null argument");
    WriterLock lk(e);
    *out_id = add_caveat_instance(e, std::string(name, name_len), std::string(json ? json : "", json_len));
  });
}

int gck_evaluate_caveat(gck_engine* ge, const char* name, size_t name_len, const char* stored_json,
                        size_t stored_len, const char* context_json, size_t context_len, uint8_t* out) {
  return guard([&] {
    Engine& e = need(ge);
    Schema& sc = need_schema(e);
    REQUIRE(name && out, GCK_E_INVALID_ARGUMENT, "null argument");
    auto cd = sc.caveats.find(std::string(name, name_len));
    REQUIRE(cd != sc.caveats.end(), GCK_E_NOT_FOUND, "unknown caveat '" + std::string(name, name_len) + "'");
    const cel::Object st = cel::parse_context(std::string(stored_json ? stored_json : "", stored_json ? stored_len : 0));
    const cel::Object cx = cel::parse_context(std::string(context_json ? context_json : "", context_json ? context_len : 0));
    *out = (uint8_t)cel::evaluate(*cd->second.expr, &st, &cx);
  });
}

int gck_begin_snapshot(gck_engine* ge, uint64_t revision) {
  return guard([&] {
    Engine& e = need(ge);
    need_schema(e);
    WriterLock lk(e);
    e.staging = true;
    e.staged_revision = revision;
    e.staged.clear();
    e.prebuilt.clear();
    e.seq = 0;
  });
}

int gck_add_tuples(gck_engine* ge, const gck_tuple* tuples, size_t n) {
  return guard([&] {
    Engine& e = need(ge);
    need_schema(e);
    REQUIRE(e.staging, GCK_E_STATE, "gck_begin_snapshot first");
    REQUIRE(n == 0 || tuples, GCK_E_INVALID_ARGUMENT, "null tuples");
    WriterLock lk(e);
    stage_tuples(e, tuples, n);
  });
}

int gck_add_tuples_text(gck_engine* ge, const char* text, size_t len) {
  return guard([&] {
    Engine& e = need(ge);
    need_schema(e);
    REQUIRE(e.staging, GCK_E_STATE, "gck_begin_snapshot first");
    REQUIRE(text || !len, GCK_E_INVALID_ARGUMENT, "null text");
    WriterLock lk(e);
    add_tuples_text(e, text, len);
  });
}

int gck_load_csr(gck_engine* ge, uint16_t relation, uint16_t subject_type, uint16_t subject_relation,
                 uint32_t n_rows, const uint32_t* offsets, const uint32_t* neighbours, uint64_t n_edges,
                 uint32_t mem_flags) {
  return guard([&] {
    Engine& e = need(ge);
    Schema& sc = need_schema(e);
    REQUIRE(e.staging, GCK_E_STATE, "gck_begin_snapshot first");
    REQUIRE(relation < sc.rels.size() && !sc.rels[relation].is_perm, GCK_E_INVALID_ARGUMENT,
            "gck_load_csr: not a relation");
    REQUIRE(subject_type < sc.types.size(), GCK_E_INVALID_ARGUMENT, "gck_load_csr: bad subject type");
    bool allowed = false;
    for (const Allowed& a : sc.rels[relation].allowed)
      if (a.stype == subject_type && a.srel == subject_relation) allowed = true;
    REQUIRE(allowed, GCK_E_INVALID_ARGUMENT, "gck_load_csr: subject kind not allowed by the schema");
    REQUIRE(offsets && (neighbours || !n_edges), GCK_E_INVALID_ARGUMENT, "gck_load_csr: null arrays");
    REQUIRE(n_edges < 0xFFFFFFFFull, GCK_E_CAPACITY, "gck_load_csr: more than 2^32-1 edges in one CSR");
    WriterLock lk(e);
    HostCSR h;
    h.rel = relation;
    h.stype = subject_type;
    h.srel = subject_relation;
    h.ext = false;
    h.n_rows = n_rows;
    h.n_edges = n_edges;
    if (mem_flags & GCK_MEM_DEVICE) {  // (a partitioned engine copies only what it keeps: device_upload)
      h.dev_off = offsets;
      h.dev_nbr = neighbours;
    } else {
      REQUIRE(offsets[n_rows] == n_edges && offsets[0] == 0, GCK_E_INVALID_ARGUMENT,
              "gck_load_csr: offsets do not span the neighbour array");
      if (e.part_world > 1) {  // partitioned graph: the rows and subjects this rank keeps (part_keep)
        h.off.assign((size_t)n_rows + 1, 0);
        for (uint32_t r = 0; r < n_rows; ++r) {
          for (uint32_t k = offsets[r]; k < offsets[r + 1]; ++k)
            if (part_keep(e, relation, r, neighbours[k], subject_relation)) h.nbr.push_back(neighbours[k]);
          h.off[r + 1] = (uint32_t)h.nbr.size();
        }
        h.n_edges = h.nbr.size();
      } else {
        h.off.assign(offsets, offsets + (size_t)n_rows + 1);
        h.nbr.assign(neighbours, neighbours + n_edges);
      }
    }
    e.prebuilt.push_back(std::move(h));
  });
}

int gck_commit_snapshot(gck_engine* ge) {
  return guard([&] {
    Engine& e = need(ge);
    need_schema(e);
    REQUIRE(e.staging, GCK_E_STATE, "gck_begin_snapshot first");
    WriterLock lk(e);
    drain_batches(e);
    std::vector<HostCSR> csrs = build_csrs(e);
    device_upload(e, csrs);  // device-pointer CSRs are copied before the caller regains control
    ensure_pool(e);          // no check ever creates a workspace (engine.hip ensure_pool)
    e.staged.clear();
    e.staged.shrink_to_fit();
    e.staging = false;
    e.revision = e.staged_revision;
    e.committed = true;
  });
}

int gck_save_snapshot(gck_engine* ge, const char* path) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(path, GCK_E_INVALID_ARGUMENT, "null path");
    WriterLock lk(e);  // no Watch batch may move the snapshot meanwhile
    save_snapshot_file(e, path);
  });
}

int gck_load_snapshot_file(gck_engine* ge, const char* path) {
  return guard([&] {
    Engine& e = need(ge);
    need_schema(e);
    REQUIRE(path, GCK_E_INVALID_ARGUMENT, "null path");
    WriterLock lk(e);
    drain_batches(e);
    load_snapshot_file(e, path);
    ensure_pool(e);
  });
}

int gck_revision(gck_engine* ge, uint64_t* out) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(out, GCK_E_INVALID_ARGUMENT, "null out");
    std::shared_lock<std::shared_mutex> lk(e.mu);
    *out = e.revision;
  });
}

int gck_set_head_revision(gck_engine* ge, uint64_t revision) {
  return guard([&] {
    Engine& e = need(ge);
    WriterLock lk(e);
    if (revision > e.head_revision) e.head_revision = revision;  // the head only moves forward
  });
}

int gck_tuple_count(gck_engine* ge, uint64_t* out) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(out, GCK_E_INVALID_ARGUMENT, "null out");
    *out = e.n_tuples;
  });
}

int gck_device_bytes(gck_engine* ge, uint64_t* out) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(out, GCK_E_INVALID_ARGUMENT, "null out");
    *out = device_bytes(e);
  });
}

// Watch batch: validated and grouped on the host first (nothing is applied if any update is
// rejected), then merged on the device and the next snapshot derived from it (delta.inc) BESIDE
// the checks: the engine lock is held shared meanwhile, so checks keep running on the current
// snapshot; it is taken exclusively again only to finish the batches in flight, patch the
// membership indexes and swap the snapshot in (device_apply_publish). `lk` (exclusive, with
// writer_mu held) is released and re-acquired here. A device failure loses the snapshot.
// `staged`: the batch's groups, made ahead by the stager (gck_watch_apply_staged)
static void apply_updates(Engine& e, std::unique_lock<std::shared_mutex>& lk, uint64_t revision, const gck_update* ups,
                          size_t n, const std::vector<UpdateGroup>* staged = nullptr) {
  REQUIRE(e.committed, GCK_E_STATE, "no snapshot committed");
  REQUIRE(revision > e.revision || (n == 0 && revision == e.revision), GCK_E_REVISION,
          "update revision " + std::to_string(revision) + " is not newer than the snapshot's " +
              std::to_string(e.revision));
  PhaseClock pc("watch");
  std::vector<gck_update> mine;
  if (e.part_world > 1 && !staged) {  // partitioned graph: the updates of what this rank keeps (part_keep)
    // the whole batch validated first, as every rank validates it: an update another rank would
    // keep and reject fails the batch here too (every rank stays at the old revision)
    validate_updates(e, ups, n);
    for (size_t i = 0; i < n; ++i) {
      const gck_tuple& t = ups[i].tuple;
      if (part_keep(e, t.relation, t.resource_id, t.subject_id, t.subject_relation)) mine.push_back(ups[i]);
    }
    ups = mine.data();
    n = mine.size();
  }
  // validation and grouping read the interner and the schema, which only writers change (and
  // writer_mu holds them off): beside the checks too
  WatchBuild wb;
  lk.unlock();
  bool built = false;
  try {
    std::shared_lock<std::shared_mutex> sl(e.mu);  // (checks run on the current snapshot meanwhile)
    // (the engine's, until the next batch; or the staged batch's)
    const std::vector<UpdateGroup>& groups = staged ? *staged : group_updates(e, ups, n);
    pc.mark("group");
    if (!groups.empty()) device_apply_build(e, groups, wb);
    built = true;
  } catch (...) {
    lk.lock();
    if (!built && !wb.ds && wb.fresh.empty()) throw;  // rejected before anything was built: nothing lost
    device_apply_abort(e, wb);
    e.committed = false;
    throw;
  }
  pc.mark("build");
  lk.lock();
  try {
    device_apply_publish(e, wb);
    pc.mark("publish");
  } catch (...) {
    device_apply_abort(e, wb);
    e.committed = false;
    throw;
  }
  e.revision = revision;
}

int gck_apply_updates(gck_engine* ge, uint64_t revision, const gck_update* updates, size_t n) {
  return guard([&] {
    Engine& e = need(ge);
    need_schema(e);
    REQUIRE(n == 0 || updates, GCK_E_INVALID_ARGUMENT, "null updates");
    PhaseClock pc("watch_call");
    {
      WriterLock wl(e);
      pc.mark("lock");
      // (read in place: no copy of the batch)
      apply_updates(e, wl.lk, revision, updates, n);
      pc.mark("apply");
    }
    pc.mark("unlock");
  });
}

// The CPUs of a sysfs cpu list ("0-7,64-71").
static std::vector<int> cpu_list(const char* path) {
  std::vector<int> out;
  FILE* f = std::fopen(path, "r");
  if (!f) return out;
  char buf[4096];
  const size_t n = std::fread(buf, 1, sizeof(buf) - 1, f);
  std::fclose(f);
  buf[n] = 0;
  for (char* p = buf; *p;) {
    char* end;
    const long a = std::strtol(p, &end, 10);
    if (end == p) break;
    long b = a;
    if (*end == '-') b = std::strtol(end + 1, &end, 10);
    for (long c = a; c <= b && c < 65536; ++c) out.push_back((int)c);
    p = *end ? end + 1 : end;
  }
  return out;
}

// Places the stager on the applying thread's last-level cache (its L3 domain minus its own core):
// the applying thread reads every record the stager wrote, which then stays in that cache instead
// of crossing between core complexes (config 5: ~30 us of a 0.2 ms step). Left to the scheduler
// when the topology cannot be read.
static void stager_place(int caller_cpu) {
  if (caller_cpu < 0) return;
  char path[128];
  std::snprintf(path, sizeof(path), "/sys/devices/system/cpu/cpu%d/cache/index3/shared_cpu_list", caller_cpu);
  std::vector<int> l3 = cpu_list(path);
  std::snprintf(path, sizeof(path), "/sys/devices/system/cpu/cpu%d/topology/thread_siblings_list", caller_cpu);
  const std::vector<int> sib = cpu_list(path);
  cpu_set_t allowed;
  if (l3.empty() || sched_getaffinity(0, sizeof(allowed), &allowed) != 0) return;
  cpu_set_t set;
  CPU_ZERO(&set);
  int n = 0;
  for (int c : l3)
    if (c < CPU_SETSIZE && CPU_ISSET(c, &allowed) && std::find(sib.begin(), sib.end(), c) == sib.end()) {
      CPU_SET(c, &set);
      ++n;
    }
  if (n) (void)pthread_setaffinity_np(pthread_self(), sizeof(set), &set);
}

// The stager's thread: groups the queued batches in ticket order.
static void stager_loop(gck_engine* ge, int caller_cpu) {
  if (!debug_env("GCK_STAGER_ANYWHERE")) stager_place(caller_cpu);
  Engine& e = ge->impl;
  WatchStager& st = ge->stage;
  std::unique_lock<std::mutex> g(st.m);
  for (;;) {
    WatchStager::Slot* s = nullptr;
    for (;;) {
      for (WatchStager::Slot& x : st.slots)
        if (x.state == 1 && (!s || x.ticket < s->ticket)) s = &x;
      if (s || st.stop) break;
      st.cv_job.wait(g);
    }
    if (!s) return;
    s->state = 3;  // (the other thread takes the next queued one)
    const gck_update* ups = s->ups;
    size_t n = s->n;
    g.unlock();
    bool ok = false;
    uint64_t gen = 0;
    const std::vector<UpdateGroup>* groups = nullptr;
    try {
      bool part;
      {
        std::shared_lock<std::shared_mutex> sl(e.mu);
        gen = e.shape_gen;
        part = e.part_world > 1;
        if (part) {  // (as apply_updates: the whole batch validated, then this rank's updates kept)
          validate_updates(e, ups, n);
          s->mine.clear();
          for (size_t i = 0; i < n; ++i) {
            const gck_tuple& t = ups[i].tuple;
            if (part_keep(e, t.relation, t.resource_id, t.subject_id, t.subject_relation)) s->mine.push_back(ups[i]);
          }
        }
      }
      if (part) {
        ups = s->mine.data();
        n = s->mine.size();
      }
      groups = &group_updates(e, s->buf, ups, n, &e.mu);
      ok = true;
    } catch (...) {
      ok = false;  // (gck_watch_apply_staged regroups it under the writer lock and reports the error)
    }
    g.lock();
    s->ok = ok;
    s->gen = gen;
    s->groups = groups;
    s->state = 2;
    st.cv_done.notify_all();
  }
}

int gck_watch_stage(gck_engine* ge, const gck_update* updates, size_t n, uint64_t* ticket) {
  return guard([&] {
    Engine& e = need(ge);
    need_schema(e);
    REQUIRE(ticket && (n == 0 || updates), GCK_E_INVALID_ARGUMENT, "null argument");
    WatchStager& st = ge->stage;
    std::lock_guard<std::mutex> g(st.m);
    WatchStager::Slot* s = nullptr;
    for (WatchStager::Slot& x : st.slots)
      if (!x.ticket) {
        s = &x;
        break;
      }
    REQUIRE(s, GCK_E_CAPACITY, "every staging slot holds a batch: apply or discard one first");
    for (std::thread& t : st.th)
      if (!t.joinable()) t = std::thread(stager_loop, ge, sched_getcpu());
    s->ups = updates;
    s->n = n;
    s->ticket = st.next_ticket++;
    s->state = 1;
    s->ok = false;
    s->groups = nullptr;
    *ticket = s->ticket;
    st.cv_job.notify_all();
  });
}

// Waits for the staged batch and frees its slot afterwards (whatever happens)
struct StagedSlot {
  WatchStager& st;
  WatchStager::Slot* s = nullptr;
  StagedSlot(WatchStager& w, uint64_t ticket) : st(w) {
    std::unique_lock<std::mutex> g(st.m);
    for (WatchStager::Slot& x : st.slots)
      if (ticket && x.ticket == ticket) s = &x;
    if (!s) throw Error(GCK_E_INVALID_ARGUMENT, "no staged Watch batch with ticket " + std::to_string(ticket));
    st.cv_done.wait(g, [&] { return s->state == 2; });
  }
  ~StagedSlot() {
    std::lock_guard<std::mutex> g(st.m);
    s->ticket = 0;
    s->state = 0;
    s->groups = nullptr;
  }
};

int gck_watch_apply_staged(gck_engine* ge, uint64_t revision, uint64_t ticket) {
  return guard([&] {
    Engine& e = need(ge);
    need_schema(e);
    StagedSlot ss(ge->stage, ticket);
    PhaseClock pc("watch_call");
    WriterLock wl(e);
    pc.mark("lock");
    // grouped against the engine's current shape: applied as staged; else (a write moved the
    // shape since, or the staging failed) grouped again here, where any error is reported
    if (ss.s->ok && ss.s->gen == e.shape_gen)
      apply_updates(e, wl.lk, revision, ss.s->ups, ss.s->n, ss.s->groups);
    else
      apply_updates(e, wl.lk, revision, ss.s->ups, ss.s->n);
    pc.mark("apply");
  });
}

int gck_watch_discard(gck_engine* ge, uint64_t ticket) {
  return guard([&] {
    need(ge);
    StagedSlot ss(ge->stage, ticket);
  });
}

// What a text Watch batch may add before it is known to apply: new interned ids (CREATE of an
// unseen object) and new caveat instances. A rejected batch takes them back, so that nothing of
// it stays (interner counts are also the CSR row counts of the next batch).
struct InternMark {
  std::vector<uint32_t> counts;
  size_t n_cav = 0, n_partial = 0;
};

static InternMark intern_mark(const Engine& e) {
  InternMark m;
  for (const TypeInterner& ti : e.interner) m.counts.push_back(ti.count);
  m.n_cav = e.caveat_instances.size();
  m.n_partial = e.caveat_partial.size();
  return m;
}

static void intern_rollback(Engine& e, const InternMark& m) {
  ++e.shape_gen;
  for (size_t t = 0; t < m.counts.size() && t < e.interner.size(); ++t) {
    TypeInterner& ti = e.interner[t];
    for (uint32_t id = m.counts[t]; id < ti.names.size(); ++id)
      if (!ti.names[id].empty()) ti.ids.erase(ti.names[id]);
    if (ti.names.size() > m.counts[t]) ti.names.resize(m.counts[t]);
    ti.count = m.counts[t];
  }
  for (size_t id = m.n_cav; id < e.caveat_instances.size(); ++id) {
    std::string key = e.caveat_instances[id].first;  // add_caveat_instance's key
    key += '\0';
    key += e.caveat_instances[id].second;
    e.caveat_ids.erase(key);
  }
  e.caveat_instances.resize(m.n_cav);
  e.caveat_expr.resize(m.n_cav);
  e.caveat_ctx.resize(m.n_cav);
  e.caveat_static.resize(m.n_cav);
  e.caveat_row.resize(m.n_cav);
  e.caveat_partial.resize(m.n_partial);
}

int gck_apply_updates_text(gck_engine* ge, uint64_t revision, const char* text, size_t len) {
  return guard([&] {
    Engine& e = need(ge);
    need_schema(e);
    REQUIRE(text || !len, GCK_E_INVALID_ARGUMENT, "null text");
    WriterLock wl(e);
    REQUIRE(e.committed, GCK_E_STATE, "no snapshot committed");
    // the revision first: a stale batch is refused before its text is read
    REQUIRE(revision > e.revision || (len == 0 && revision == e.revision), GCK_E_REVISION,
            "update revision " + std::to_string(revision) + " is not newer than the snapshot's " +
                std::to_string(e.revision));
    drain_batches(e);
    const InternMark mark = intern_mark(e);
    try {
      std::vector<gck_update> ups;
      parse_updates_text(e, text, len, ups);
      apply_updates(e, wl.lk, revision, ups.data(), ups.size());
    } catch (...) {
      intern_rollback(e, mark);  // (apply_updates returns or throws with the lock held)
      throw;
    }
  });
}

// consistency.Strategy (consistency/consistency.go:15-77) against the applied revision. A
// requirement the snapshot has not reached yet is GCK_E_REVISION (gRPC Unavailable: the client
// retries, client/client.go:193-211, while the Watch stream catches up); a Snapshot revision the
// snapshot has moved past can never be served here (no MVCC on the device) and is permanent.
static void check_consistency(Engine& e, const gck_consistency* cs) {
  if (!cs) return;
  switch (cs->requirement) {
    case GCK_CONSISTENCY_MIN_LATENCY:
      return;
    case GCK_CONSISTENCY_FULL:
      REQUIRE(e.revision >= e.head_revision, GCK_E_REVISION,
              "snapshot revision " + std::to_string(e.revision) + " has not reached the head revision " +
                  std::to_string(e.head_revision));
      return;
    case GCK_CONSISTENCY_AT_LEAST:
      REQUIRE(e.revision >= cs->revision, GCK_E_REVISION,
              "snapshot revision " + std::to_string(e.revision) + " is older than the requested " +
                  std::to_string(cs->revision));
      return;
    case GCK_CONSISTENCY_SNAPSHOT:
      REQUIRE(e.revision <= cs->revision, GCK_E_REVISION_GONE,
              "snapshot revision " + std::to_string(cs->revision) + " is no longer available (the local snapshot is at " +
                  std::to_string(e.revision) + ")");
      REQUIRE(e.revision == cs->revision, GCK_E_REVISION,
              "snapshot revision " + std::to_string(e.revision) + " has not reached the requested " +
                  std::to_string(cs->revision));
      return;
    default:
      throw Error(GCK_E_INVALID_ARGUMENT, "unknown consistency requirement");
  }
}

// State errors before any workspace is taken (a workspace needs the device the first commit set
// up): no snapshot, or a partitioned engine.
static void precheck(Engine& e) {
  std::shared_lock<std::shared_mutex> lk(e.mu);
  REQUIRE(e.committed, GCK_E_STATE, "no snapshot committed");
  REQUIRE(e.part_world <= 1, GCK_E_STATE, "partitioned engine: use gck_part_* (every rank together)");
}

// The checks common to every check entry point (under the shared engine lock).
// (A host item's context_slot is validated by its batch: the join of a zero-copy batch checks every
// item it reads, the others are scanned before they are staged — engine.hip submit_batch; a scan
// here read every host item once more on the submitting thread, ~27 us per 64K batch.)
static void check_request(Engine& e, const gck_consistency* cs, const char* const* contexts, const size_t* context_lens,
                          size_t n_contexts) {
  REQUIRE(e.committed, GCK_E_STATE, "no snapshot committed");
  REQUIRE(n_contexts == 0 || (contexts && context_lens), GCK_E_INVALID_ARGUMENT, "null contexts");
  REQUIRE(n_contexts < 0xFFFFFFFFull, GCK_E_INVALID_ARGUMENT, "too many contexts");
  REQUIRE(e.part_world <= 1, GCK_E_STATE, "partitioned engine: use gck_part_* (every rank together)");
  check_consistency(e, cs);
}

// What a check call says beside its request: the consistency it asks for and its caveat contexts.
struct CallCtx {
  const gck_consistency* cs;
  const char* const* contexts;
  const size_t* context_lens;
  size_t n_contexts;
};

// A synchronous call over host buffers, after the entry point's own argument checks: a request of
// n checks in chunks of `chunk`; run(w0, w1, cav) checks it and writes the results.
extern "C++" {  // (a template cannot have C linkage)
template <class Run>
static void check_sync(Engine& e, const CallCtx& c, size_t n, size_t chunk, uint64_t* out_revision, Run run) {
  if (n == 0) {  // empty request -> empty response (client/client_test.go:203-207): no workspace
    std::shared_lock<std::shared_mutex> lk(e.mu);
    check_request(e, c.cs, c.contexts, c.context_lens, c.n_contexts);
    if (out_revision) *out_revision = e.revision;
    return;
  }
  // workspaces first, then the engine lock (engine.hpp WsLease)
  precheck(e);
  // a request above the chunk size alternates over two workspaces, taken in one step (never one
  // held while waiting for the other: acquire_ws_n)
  WsPair p(e, n > chunk ? 2 : 1);
  // (the shared lock is held until the results are written: no Watch batch publishes meanwhile,
  // so the revision read here is the one every chunk runs on)
  std::shared_lock<std::shared_mutex> lk(e.mu);
  check_request(e, c.cs, c.contexts, c.context_lens, c.n_contexts);
  const CavCall cav = caveat_call(e, c.contexts, c.context_lens, c.n_contexts);
  const uint64_t rev = e.revision;
  run(p.ws[0], p.ws[1], cav);
  if (out_revision) *out_revision = rev;
}
}  // extern "C++"

static size_t max_batch_of(const Engine& e) { return e.cfg.max_batch ? e.cfg.max_batch : 65536; }

int gck_check_bulk_at(gck_engine* ge, const gck_consistency* cs, const gck_item* items, size_t n,
                      const char* const* contexts, const size_t* context_lens, size_t n_contexts,
                      int64_t now_us, uint8_t* out_perm, int32_t* out_err, uint64_t* out_revision) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(n == 0 || (items && out_perm && out_err), GCK_E_INVALID_ARGUMENT, "null buffers");
    check_sync(e, {cs, contexts, context_lens, n_contexts}, n, max_batch_of(e), out_revision,
               [&](Workspace* w0, Workspace* w1, const CavCall& cav) {
                 device_check_host(e, w0, w1, items, n, now_us, out_perm, out_err, cav);
               });
  });
}

int gck_check_bulk_ctx(gck_engine* ge, const gck_consistency* cs, const gck_item* items, size_t n,
                       const char* const* contexts, const size_t* context_lens, size_t n_contexts,
                       int64_t now_us, uint8_t* out_perm, int32_t* out_err) {
  return gck_check_bulk_at(ge, cs, items, n, contexts, context_lens, n_contexts, now_us, out_perm, out_err, nullptr);
}

int gck_check_bulk(gck_engine* ge, const gck_consistency* cs, const gck_item* items, size_t n,
                   int64_t now_us, uint8_t* out_perm, int32_t* out_err) {
  return gck_check_bulk_at(ge, cs, items, n, nullptr, nullptr, 0, now_us, out_perm, out_err, nullptr);
}

// The argument checks the compact entry points share, after the header's or the table's own
// (check_uniform / check_shapes) and in the ABI's order: the buffers, the error list, then the count
// is cleared. indexed: a shaped request (its index bytes are one of the buffers). Returns the
// request as the engine takes it (engine.hpp CompactReq).
static CompactReq compact_request(const gck_uniform* shapes, size_t n_shapes, bool indexed, const uint8_t* shape_of,
                                  const uint32_t* pairs, size_t n, uint64_t* out_packed, gck_item_error* out_errs,
                                  size_t err_cap, size_t* out_n_errs) {
  REQUIRE(n == 0 || ((shape_of || !indexed) && pairs && out_packed), GCK_E_INVALID_ARGUMENT, "null buffers");
  REQUIRE(err_cap == 0 || out_errs, GCK_E_INVALID_ARGUMENT, "null error list");
  if (out_n_errs) *out_n_errs = 0;
  return CompactReq{shapes, (uint32_t)n_shapes, indexed ? shape_of : nullptr, pairs, n, out_packed, out_errs, err_cap,
                    out_n_errs};
}

// gck_check_bulk_uniform / gck_check_bulk_shaped after their argument checks (chunks: whole words).
static void check_compact_sync(Engine& e, const CallCtx& c, const CompactReq& req, int64_t now_us,
                               uint64_t* out_revision) {
  check_sync(e, c, req.n, max_batch_of(e) & ~(size_t)31, out_revision,
             [&](Workspace* w0, Workspace* w1, const CavCall& cav) { device_check_compact(e, w0, w1, req, now_us, cav); });
}

// A uniform request's header against the call (include/gck.h gck_uniform): its context slot is
// every pair's, so it is checked once here.
static void check_uniform(const gck_uniform* h, size_t n_contexts) {
  REQUIRE(h, GCK_E_INVALID_ARGUMENT, "null header");
  REQUIRE(h->context_slot <= n_contexts, GCK_E_INVALID_ARGUMENT,
          "uniform header: context_slot " + std::to_string(h->context_slot) + " beyond the " +
              std::to_string(n_contexts) + " contexts given");
}

int gck_check_bulk_uniform(gck_engine* ge, const gck_consistency* cs, const gck_uniform* hdr, const uint32_t* pairs,
                           size_t n, const char* const* contexts, const size_t* context_lens, size_t n_contexts,
                           int64_t now_us, uint64_t* out_packed, gck_item_error* out_errs, size_t err_cap,
                           size_t* out_n_errs, uint64_t* out_revision) {
  return guard([&] {
    Engine& e = need(ge);
    check_uniform(hdr, n_contexts);
    const CompactReq req = compact_request(hdr, 1, false, nullptr, pairs, n, out_packed, out_errs, err_cap, out_n_errs);
    check_compact_sync(e, {cs, contexts, context_lens, n_contexts}, req, now_us, out_revision);
  });
}

int gck_check_bulk_device_ctx(gck_engine* ge, const gck_item* d_items, size_t n, const char* const* contexts,
                              const size_t* context_lens, size_t n_contexts, int64_t now_us,
                              uint8_t* d_out_perm, int32_t* d_out_err, void* stream) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(n == 0 || (d_items && d_out_perm && d_out_err), GCK_E_INVALID_ARGUMENT, "null buffers");
    if (n == 0) {
      std::shared_lock<std::shared_mutex> lk(e.mu);
      check_request(e, nullptr, contexts, context_lens, n_contexts);
      return;
    }
    precheck(e);
    WsLease l0(e);
    std::shared_lock<std::shared_mutex> lk(e.mu);
    check_request(e, nullptr, contexts, context_lens, n_contexts);
    device_check(e, *l0.w, d_items, n, now_us, d_out_perm, d_out_err, stream,
                 caveat_call(e, contexts, context_lens, n_contexts));
  });
}

int gck_check_bulk_device(gck_engine* ge, const gck_item* d_items, size_t n, int64_t now_us,
                          uint8_t* d_out_perm, int32_t* d_out_err, void* stream) {
  return gck_check_bulk_device_ctx(ge, d_items, n, nullptr, nullptr, 0, now_us, d_out_perm, d_out_err, stream);
}

// A submitted batch: the workspace it holds (returned to the pool by the wait), or, for an empty
// batch, nothing to do.
struct gck_batch {
  Workspace* w = nullptr;
  uint64_t revision = 0;  // the snapshot's revision at submit: the one the batch runs on
};

// A submit entry point after its own argument checks: start(w, cav) queues the n checks on the
// workspace taken for them. Returns the batch; whatever throws, the workspace is back in the pool
// and the batch deleted.
extern "C++" {
template <class Start>
static gck_batch* submit_with(Engine& e, const CallCtx& c, size_t n, Start start) {
  std::unique_ptr<gck_batch> b(new gck_batch());
  if (n == 0) {  // an empty batch holds no workspace
    std::shared_lock<std::shared_mutex> lk(e.mu);
    check_request(e, c.cs, c.contexts, c.context_lens, c.n_contexts);
    b->revision = e.revision;
    return b.release();
  }
  precheck(e);
  Workspace* w = acquire_ws(e);  // before the engine lock (engine.hpp WsLease)
  try {
    std::shared_lock<std::shared_mutex> lk(e.mu);
    check_request(e, c.cs, c.contexts, c.context_lens, c.n_contexts);
    b->revision = e.revision;
    start(w, caveat_call(e, c.contexts, c.context_lens, c.n_contexts));
  } catch (...) {
    release_ws(e, w);
    throw;
  }
  b->w = w;
  return b.release();
}
}  // extern "C++"

int gck_check_submit(gck_engine* ge, const gck_consistency* cs, const gck_item* items, size_t n,
                     const char* const* contexts, const size_t* context_lens, size_t n_contexts, int64_t now_us,
                     uint8_t* out_perm, int32_t* out_err, uint32_t flags, void* stream, gck_batch** out) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(out, GCK_E_INVALID_ARGUMENT, "null out");
    *out = nullptr;
    REQUIRE(n == 0 || (items && out_perm && out_err), GCK_E_INVALID_ARGUMENT, "null buffers");
    const bool host = !(flags & GCK_SUBMIT_DEVICE);
    *out = submit_with(e, {cs, contexts, context_lens, n_contexts}, n, [&](Workspace* w, CavCall cav) {
      device_submit(e, w, items, n, now_us, out_perm, out_err, stream, host, !host && (flags & GCK_SUBMIT_ENGINE_STREAM),
                    std::move(cav));
    });
  });
}

int gck_check_submit_uniform(gck_engine* ge, const gck_consistency* cs, const gck_uniform* hdr, const uint32_t* pairs,
                             size_t n, const char* const* contexts, const size_t* context_lens, size_t n_contexts,
                             int64_t now_us, uint64_t* out_packed, gck_item_error* out_errs, size_t err_cap,
                             size_t* out_n_errs, gck_batch** out) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(out, GCK_E_INVALID_ARGUMENT, "null out");
    *out = nullptr;
    check_uniform(hdr, n_contexts);
    const CompactReq req = compact_request(hdr, 1, false, nullptr, pairs, n, out_packed, out_errs, err_cap, out_n_errs);
    *out = submit_with(e, {cs, contexts, context_lens, n_contexts}, n, [&](Workspace* w, CavCall cav) {
      device_submit_compact(e, w, req, now_us, std::move(cav));
    });
  });
}

// A shaped request's table against the call (include/gck.h gck_check_bulk_shaped): every entry is
// checked here, once; the index bytes by whoever reads them (the join in place, or the expansion).
static void check_shapes(const gck_uniform* shapes, size_t n_shapes, size_t n_contexts) {
  REQUIRE(n_shapes >= 1 && n_shapes <= GCK_MAX_SHAPES, GCK_E_INVALID_ARGUMENT,
          "shaped request: n_shapes " + std::to_string(n_shapes) + " outside 1.." + std::to_string(GCK_MAX_SHAPES));
  REQUIRE(shapes, GCK_E_INVALID_ARGUMENT, "null shape table");
  for (size_t s = 0; s < n_shapes; ++s) {
    REQUIRE(shapes[s].context_slot <= n_contexts, GCK_E_INVALID_ARGUMENT,
            "shape " + std::to_string(s) + ": context_slot " + std::to_string(shapes[s].context_slot) + " beyond the " +
                std::to_string(n_contexts) + " contexts given");
    REQUIRE(shapes[s].reserved == 0, GCK_E_INVALID_ARGUMENT, "shape " + std::to_string(s) + ": reserved must be 0");
  }
}

int gck_check_bulk_shaped(gck_engine* ge, const gck_consistency* cs, const gck_uniform* shapes, size_t n_shapes,
                          const uint8_t* shape_of, const uint32_t* pairs, size_t n, const char* const* contexts,
                          const size_t* context_lens, size_t n_contexts, int64_t now_us, uint64_t* out_packed,
                          gck_item_error* out_errs, size_t err_cap, size_t* out_n_errs, uint64_t* out_revision) {
  return guard([&] {
    Engine& e = need(ge);
    check_shapes(shapes, n_shapes, n_contexts);
    const CompactReq req =
        compact_request(shapes, n_shapes, true, shape_of, pairs, n, out_packed, out_errs, err_cap, out_n_errs);
    check_compact_sync(e, {cs, contexts, context_lens, n_contexts}, req, now_us, out_revision);
  });
}

int gck_check_submit_shaped(gck_engine* ge, const gck_consistency* cs, const gck_uniform* shapes, size_t n_shapes,
                            const uint8_t* shape_of, const uint32_t* pairs, size_t n, const char* const* contexts,
                            const size_t* context_lens, size_t n_contexts, int64_t now_us, uint64_t* out_packed,
                            gck_item_error* out_errs, size_t err_cap, size_t* out_n_errs, gck_batch** out) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(out, GCK_E_INVALID_ARGUMENT, "null out");
    *out = nullptr;
    check_shapes(shapes, n_shapes, n_contexts);
    const CompactReq req =
        compact_request(shapes, n_shapes, true, shape_of, pairs, n, out_packed, out_errs, err_cap, out_n_errs);
    *out = submit_with(e, {cs, contexts, context_lens, n_contexts}, n, [&](Workspace* w, CavCall cav) {
      device_submit_compact(e, w, req, now_us, std::move(cav));
    });
  });
}

int gck_shaped_stats(gck_engine* ge, uint64_t out[2]) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(out, GCK_E_INVALID_ARGUMENT, "null out");
    out[0] = e.shaped_in_place.load(std::memory_order_relaxed);
    out[1] = e.shaped_expanded.load(std::memory_order_relaxed);
  });
}

// ---- cross requests (include/gck.h gck_check_bulk_cross) ------------------------------------

int gck_cross_tile(size_t S, size_t R, size_t max_batch, uint32_t* rows, uint32_t* cols) {
  size_t best_rows = 0, best_cols = 0;
  // the candidate widths: every multiple of 32 up to R, and R itself; each with the most rows it
  // admits. More checks win; on a tie the wider tile.
  const auto consider = [&](size_t c) {
    if (c == 0 || c > R || c >= GCK_CROSS_IDS) return;
    const size_t r = std::min({S, max_batch / (32 * ((c + 31) / 32)), (size_t)GCK_CROSS_IDS - c});
    if (r == 0) return;
    const size_t have = best_rows * best_cols;
    if (r * c > have || (r * c == have && c > best_cols)) best_rows = r, best_cols = c;
  };
  for (size_t c = 32; c <= R && c < GCK_CROSS_IDS; c += 32) consider(c);
  consider(R);
  // the thin rule: a request of more checks than the best tile, whose best tile is small
  // (rows <= S and cols <= R: the request has more checks iff the tile is smaller in a dimension)
  const bool thin = best_rows && (S > best_rows || R > best_cols) && best_rows * best_cols < max_batch / 4;
  const bool ok = best_rows != 0 && !thin;
  if (rows) *rows = ok ? (uint32_t)best_rows : 0u;
  if (cols) *cols = ok ? (uint32_t)best_cols : 0u;
  return ok ? 1 : 0;
}

// A cross request's arguments against the call, in the ABI's order, before anything else (no
// snapshot is needed to fail them). Returns the request as the engine takes it; n = S * R.
static CompactReq cross_request(const gck_uniform* hdr, const uint32_t* subjects, size_t S, const uint32_t* resources,
                                size_t R, size_t n_contexts, uint64_t* out_packed, gck_item_error* out_errs,
                                size_t err_cap, size_t* out_n_errs) {
  check_uniform(hdr, n_contexts);
  REQUIRE(hdr->reserved == 0, GCK_E_INVALID_ARGUMENT, "cross header: reserved must be 0");
  REQUIRE(S == 0 || R == 0 || S <= 0xFFFFFFFFull / R, GCK_E_INVALID_ARGUMENT,
          "cross request: " + std::to_string(S) + " x " + std::to_string(R) + " checks reach 2^32");
  const size_t n = S * R;
  REQUIRE(n == 0 || (subjects && resources && out_packed), GCK_E_INVALID_ARGUMENT, "null buffers");
  REQUIRE(err_cap == 0 || out_errs, GCK_E_INVALID_ARGUMENT, "null error list");
  if (out_n_errs) *out_n_errs = 0;
  CompactReq q{hdr, 1u, nullptr, nullptr, n, out_packed, out_errs, err_cap, out_n_errs};
  if (n) {  // (an empty request keeps resources null: it takes the empty uniform request's path)
    q.subjects = subjects;
    q.resources = resources;
    q.S = S;
    q.R = R;
  }
  return q;
}

int gck_check_bulk_cross(gck_engine* ge, const gck_consistency* cs, const gck_uniform* hdr, const uint32_t* subjects,
                         size_t n_subjects, const uint32_t* resources, size_t n_resources, const char* const* contexts,
                         const size_t* context_lens, size_t n_contexts, int64_t now_us, uint64_t* out_packed,
                         gck_item_error* out_errs, size_t err_cap, size_t* out_n_errs, uint64_t* out_revision) {
  return guard([&] {
    Engine& e = need(ge);
    const CompactReq req = cross_request(hdr, subjects, n_subjects, resources, n_resources, n_contexts, out_packed,
                                         out_errs, err_cap, out_n_errs);
    // two workspaces when the request is more than one batch either way: more than one tile, or
    // (expanded) more than max_batch checks
    uint32_t rows = 0, cols = 0;
    const size_t mb = max_batch_of(e);
    const size_t one = gck_cross_tile(n_subjects, n_resources, mb, &rows, &cols) ? std::min(mb, (size_t)rows * cols) : mb;
    check_sync(e, {cs, contexts, context_lens, n_contexts}, req.n, one, out_revision,
               [&](Workspace* w0, Workspace* w1, const CavCall& cav) { device_check_compact(e, w0, w1, req, now_us, cav); });
  });
}

int gck_check_submit_cross(gck_engine* ge, const gck_consistency* cs, const gck_uniform* hdr, const uint32_t* subjects,
                           size_t n_subjects, const uint32_t* resources, size_t n_resources,
                           const char* const* contexts, const size_t* context_lens, size_t n_contexts, int64_t now_us,
                           uint64_t* out_packed, gck_item_error* out_errs, size_t err_cap, size_t* out_n_errs,
                           gck_batch** out) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(out, GCK_E_INVALID_ARGUMENT, "null out");
    *out = nullptr;
    const CompactReq req = cross_request(hdr, subjects, n_subjects, resources, n_resources, n_contexts, out_packed,
                                         out_errs, err_cap, out_n_errs);
    uint32_t rows = 0, cols = 0;
    REQUIRE(req.n == 0 || (gck_cross_tile(n_subjects, n_resources, max_batch_of(e), &rows, &cols) && rows == n_subjects &&
                           cols == n_resources),
            GCK_E_INVALID_ARGUMENT,
            "submitted cross request of " + std::to_string(n_subjects) + " x " + std::to_string(n_resources) +
                " is not one tile (gck_cross_tile)");
    *out = submit_with(e, {cs, contexts, context_lens, n_contexts}, req.n, [&](Workspace* w, CavCall cav) {
      device_submit_compact(e, w, req, now_us, std::move(cav));
    });
  });
}

int gck_cross_stats(gck_engine* ge, uint64_t out[2]) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(out, GCK_E_INVALID_ARGUMENT, "null out");
    out[0] = e.cross_in_place.load(std::memory_order_relaxed);
    out[1] = e.cross_expanded.load(std::memory_order_relaxed);
  });
}

// ---- list requests (include/gck.h gck_check_bulk_list) ---------------------------------------

// A list request's arguments against the call, in the ABI's order, before anything else (no snapshot
// is needed to fail them). Returns the request as the engine takes it.
static CompactReq list_request(const gck_uniform* hdr, uint32_t fixed_id, uint32_t vary, const uint32_t* ids,
                               uint32_t first_id, size_t n, size_t n_contexts, uint64_t* out_packed,
                               gck_item_error* out_errs, size_t err_cap, size_t* out_n_errs,
                               bool need_plane = true) {
  check_uniform(hdr, n_contexts);
  REQUIRE(hdr->reserved == 0, GCK_E_INVALID_ARGUMENT, "list header: reserved must be 0");
  REQUIRE(vary == GCK_VARY_RESOURCE || vary == GCK_VARY_SUBJECT, GCK_E_INVALID_ARGUMENT,
          "list request: vary must be GCK_VARY_RESOURCE or GCK_VARY_SUBJECT");
  if (!ids && n) {
    REQUIRE(vary == GCK_VARY_RESOURCE, GCK_E_INVALID_ARGUMENT,
            "list request: a range varies the resource id (the fixed id is the subject's)");
    REQUIRE((uint64_t)first_id + n <= 0x100000000ull, GCK_E_INVALID_ARGUMENT,
            "list request: the range " + std::to_string(first_id) + " + " + std::to_string(n) + " passes 2^32");
  }
  REQUIRE(n == 0 || out_packed || !need_plane, GCK_E_INVALID_ARGUMENT, "null buffers");
  REQUIRE(err_cap == 0 || out_errs, GCK_E_INVALID_ARGUMENT, "null error list");
  if (out_n_errs) *out_n_errs = 0;
  CompactReq q{hdr, 1u, nullptr, nullptr, n, out_packed, out_errs, err_cap, out_n_errs};
  q.vary = vary;
  q.fixed_id = fixed_id;
  q.first_id = ids ? 0u : first_id;
  q.ids = ids;
  return q;
}

int gck_check_bulk_list(gck_engine* ge, const gck_consistency* cs, const gck_uniform* hdr, uint32_t fixed_id,
                        uint32_t vary, const uint32_t* ids, uint32_t first_id, size_t n, const char* const* contexts,
                        const size_t* context_lens, size_t n_contexts, int64_t now_us, uint64_t* out_packed,
                        gck_item_error* out_errs, size_t err_cap, size_t* out_n_errs, uint64_t* out_revision) {
  return guard([&] {
    Engine& e = need(ge);
    const CompactReq req =
        list_request(hdr, fixed_id, vary, ids, first_id, n, n_contexts, out_packed, out_errs, err_cap, out_n_errs);
    check_compact_sync(e, {cs, contexts, context_lens, n_contexts}, req, now_us, out_revision);
  });
}

int gck_check_submit_list(gck_engine* ge, const gck_consistency* cs, const gck_uniform* hdr, uint32_t fixed_id,
                          uint32_t vary, const uint32_t* ids, uint32_t first_id, size_t n, const char* const* contexts,
                          const size_t* context_lens, size_t n_contexts, int64_t now_us, uint64_t* out_packed,
                          gck_item_error* out_errs, size_t err_cap, size_t* out_n_errs, gck_batch** out) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(out, GCK_E_INVALID_ARGUMENT, "null out");
    *out = nullptr;
    const CompactReq req =
        list_request(hdr, fixed_id, vary, ids, first_id, n, n_contexts, out_packed, out_errs, err_cap, out_n_errs);
    *out = submit_with(e, {cs, contexts, context_lens, n_contexts}, n, [&](Workspace* w, CavCall cav) {
      device_submit_compact(e, w, req, now_us, std::move(cav));
    });
  });
}

int gck_list_stats(gck_engine* ge, uint64_t out[2]) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(out, GCK_E_INVALID_ARGUMENT, "null out");
    out[0] = e.list_in_place.load(std::memory_order_relaxed);
    out[1] = e.list_expanded.load(std::memory_order_relaxed);
  });
}

// ---- compact requests over device buffers (include/gck.h gck_check_bulk_uniform_device) ------

// What the device forms check beyond their host forms, before anything is launched, and the request
// as the engine takes it: `q` is the host form's request built over the device pointers (its checks
// have passed; none of them reads a buffer).
static CompactReq device_request(CompactReq q, const void* d_errs, uint32_t* d_n_errs, void* stream,
                                 bool engine_stream) {
  const auto aligned = [](const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; };
  REQUIRE(q.n < 0x100000000ull, GCK_E_INVALID_ARGUMENT, "device request: " + std::to_string(q.n) + " checks reach 2^32");
  REQUIRE(aligned(q.pairs, 8), GCK_E_INVALID_ARGUMENT, "device request: d_pairs is not 8-byte aligned");
  REQUIRE(aligned(q.packed, 8), GCK_E_INVALID_ARGUMENT, "device request: d_out_packed is not 8-byte aligned");
  REQUIRE(aligned(q.ids, 4), GCK_E_INVALID_ARGUMENT, "device request: d_ids is not 4-byte aligned");
  REQUIRE(aligned(d_errs, 4), GCK_E_INVALID_ARGUMENT, "device request: d_out_errs is not 4-byte aligned");
  REQUIRE(aligned(d_n_errs, 4), GCK_E_INVALID_ARGUMENT, "device request: d_out_n_errs is not 4-byte aligned");
  q.device = true;
  q.engine_stream = engine_stream;
  q.stream = stream;
  q.d_n_errs = d_n_errs;
  return q;
}

// A synchronous device request after its argument checks: an empty one clears the count and takes
// no workspace.
static void check_device_sync(Engine& e, const CallCtx& c, const CompactReq& req, int64_t now_us,
                              uint64_t* out_revision) {
  if (req.n == 0) {
    std::shared_lock<std::shared_mutex> lk(e.mu);
    check_request(e, c.cs, c.contexts, c.context_lens, c.n_contexts);
    device_zero_count(e, req.d_n_errs, req.stream);
    if (req.sel) device_zero_count(e, req.sel->d_out_n, req.stream);
    if (out_revision) *out_revision = e.revision;
    return;
  }
  check_compact_sync(e, c, req, now_us, out_revision);
}

// ... and a submitted one (flags: GCK_SUBMIT_ENGINE_STREAM or the caller's stream; GCK_SUBMIT_DEVICE is implied).
static gck_batch* submit_device(Engine& e, const CallCtx& c, const CompactReq& req, int64_t now_us) {
  gck_batch* b = submit_with(e, c, req.n, [&](Workspace* w, CavCall cav) {
    device_submit_compact(e, w, req, now_us, std::move(cav));
  });
  if (req.n == 0) {
    try {
      device_zero_count(e, req.d_n_errs, req.engine_stream ? nullptr : req.stream);
      if (req.sel) device_zero_count(e, req.sel->d_out_n, req.engine_stream ? nullptr : req.stream);
    } catch (...) {
      delete b;
      throw;
    }
  }
  return b;
}

static void check_submit_flags(uint32_t flags) {
  REQUIRE(!(flags & ~(GCK_SUBMIT_DEVICE | GCK_SUBMIT_ENGINE_STREAM)), GCK_E_INVALID_ARGUMENT, "unknown submit flags");
}

int gck_check_bulk_uniform_device(gck_engine* ge, const gck_consistency* cs, const gck_uniform* hdr,
                                  const uint32_t* d_pairs, size_t n, const char* const* contexts,
                                  const size_t* context_lens, size_t n_contexts, int64_t now_us, uint64_t* d_out_packed,
                                  gck_item_error* d_out_errs, size_t err_cap, uint32_t* d_out_n_errs, void* stream,
                                  uint64_t* out_revision) {
  return guard([&] {
    Engine& e = need(ge);
    check_uniform(hdr, n_contexts);
    const CompactReq req =
        device_request(compact_request(hdr, 1, false, nullptr, d_pairs, n, d_out_packed, d_out_errs, err_cap, nullptr),
                       d_out_errs, d_out_n_errs, stream, true);
    check_device_sync(e, {cs, contexts, context_lens, n_contexts}, req, now_us, out_revision);
  });
}

int gck_check_submit_uniform_device(gck_engine* ge, const gck_consistency* cs, const gck_uniform* hdr,
                                    const uint32_t* d_pairs, size_t n, const char* const* contexts,
                                    const size_t* context_lens, size_t n_contexts, int64_t now_us,
                                    uint64_t* d_out_packed, gck_item_error* d_out_errs, size_t err_cap,
                                    uint32_t* d_out_n_errs, uint32_t flags, void* stream, gck_batch** out) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(out, GCK_E_INVALID_ARGUMENT, "null out");
    *out = nullptr;
    check_submit_flags(flags);
    check_uniform(hdr, n_contexts);
    const CompactReq req =
        device_request(compact_request(hdr, 1, false, nullptr, d_pairs, n, d_out_packed, d_out_errs, err_cap, nullptr),
                       d_out_errs, d_out_n_errs, stream, (flags & GCK_SUBMIT_ENGINE_STREAM) != 0);
    *out = submit_device(e, {cs, contexts, context_lens, n_contexts}, req, now_us);
  });
}

int gck_check_bulk_shaped_device(gck_engine* ge, const gck_consistency* cs, const gck_uniform* shapes, size_t n_shapes,
                                 const uint8_t* d_shape_of, const uint32_t* d_pairs, size_t n,
                                 const char* const* contexts, const size_t* context_lens, size_t n_contexts,
                                 int64_t now_us, uint64_t* d_out_packed, gck_item_error* d_out_errs, size_t err_cap,
                                 uint32_t* d_out_n_errs, void* stream, uint64_t* out_revision) {
  return guard([&] {
    Engine& e = need(ge);
    check_shapes(shapes, n_shapes, n_contexts);
    const CompactReq req = device_request(
        compact_request(shapes, n_shapes, true, d_shape_of, d_pairs, n, d_out_packed, d_out_errs, err_cap, nullptr),
        d_out_errs, d_out_n_errs, stream, true);
    check_device_sync(e, {cs, contexts, context_lens, n_contexts}, req, now_us, out_revision);
  });
}

int gck_check_submit_shaped_device(gck_engine* ge, const gck_consistency* cs, const gck_uniform* shapes,
                                   size_t n_shapes, const uint8_t* d_shape_of, const uint32_t* d_pairs, size_t n,
                                   const char* const* contexts, const size_t* context_lens, size_t n_contexts,
                                   int64_t now_us, uint64_t* d_out_packed, gck_item_error* d_out_errs, size_t err_cap,
                                   uint32_t* d_out_n_errs, uint32_t flags, void* stream, gck_batch** out) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(out, GCK_E_INVALID_ARGUMENT, "null out");
    *out = nullptr;
    check_submit_flags(flags);
    check_shapes(shapes, n_shapes, n_contexts);
    const CompactReq req = device_request(
        compact_request(shapes, n_shapes, true, d_shape_of, d_pairs, n, d_out_packed, d_out_errs, err_cap, nullptr),
        d_out_errs, d_out_n_errs, stream, (flags & GCK_SUBMIT_ENGINE_STREAM) != 0);
    *out = submit_device(e, {cs, contexts, context_lens, n_contexts}, req, now_us);
  });
}

int gck_check_bulk_list_device(gck_engine* ge, const gck_consistency* cs, const gck_uniform* hdr, uint32_t fixed_id,
                               uint32_t vary, const uint32_t* d_ids, uint32_t first_id, size_t n,
                               const char* const* contexts, const size_t* context_lens, size_t n_contexts,
                               int64_t now_us, uint64_t* d_out_packed, gck_item_error* d_out_errs, size_t err_cap,
                               uint32_t* d_out_n_errs, void* stream, uint64_t* out_revision) {
  return guard([&] {
    Engine& e = need(ge);
    const CompactReq req = device_request(
        list_request(hdr, fixed_id, vary, d_ids, first_id, n, n_contexts, d_out_packed, d_out_errs, err_cap, nullptr),
        d_out_errs, d_out_n_errs, stream, true);
    check_device_sync(e, {cs, contexts, context_lens, n_contexts}, req, now_us, out_revision);
  });
}

int gck_check_submit_list_device(gck_engine* ge, const gck_consistency* cs, const gck_uniform* hdr, uint32_t fixed_id,
                                 uint32_t vary, const uint32_t* d_ids, uint32_t first_id, size_t n,
                                 const char* const* contexts, const size_t* context_lens, size_t n_contexts,
                                 int64_t now_us, uint64_t* d_out_packed, gck_item_error* d_out_errs, size_t err_cap,
                                 uint32_t* d_out_n_errs, uint32_t flags, void* stream, gck_batch** out) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(out, GCK_E_INVALID_ARGUMENT, "null out");
    *out = nullptr;
    check_submit_flags(flags);
    const CompactReq req = device_request(
        list_request(hdr, fixed_id, vary, d_ids, first_id, n, n_contexts, d_out_packed, d_out_errs, err_cap, nullptr),
        d_out_errs, d_out_n_errs, stream, (flags & GCK_SUBMIT_ENGINE_STREAM) != 0);
    *out = submit_device(e, {cs, contexts, context_lens, n_contexts}, req, now_us);
  });
}

// ---- cross requests over device buffers (include/gck.h gck_check_bulk_cross_device) -----------

int gck_cross_tile_device(size_t S, size_t R, size_t max_batch, uint32_t* rows) {
  if (rows) *rows = 0;
  if (S == 0 || R == 0 || R >= GCK_CROSS_IDS) return 0;
  const size_t padded = 32 * ((R + 31) / 32);  // a row's checks, padding included
  if (padded > max_batch) return 0;
  const size_t r = std::min({S, max_batch / padded, (size_t)GCK_CROSS_IDS - R});
  if (r == 0) return 0;
  // gck_cross_tile's thin rule: more checks than the tile, and the tile is small
  if (S > r && r * R < max_batch / 4) return 0;
  if (rows) *rows = (uint32_t)r;
  return 1;
}

// The host cross call's argument checks over the device pointers (none reads a buffer), then the
// device forms' own.
static CompactReq cross_device_request(const gck_uniform* hdr, const uint32_t* d_subjects, size_t S,
                                       const uint32_t* d_resources, size_t R, size_t n_contexts, uint64_t* d_out_packed,
                                       gck_item_error* d_out_errs, size_t err_cap, uint32_t* d_out_n_errs, void* stream,
                                       bool engine_stream) {
  const auto aligned = [](const void* p) { return ((uintptr_t)p & 3u) == 0; };
  const CompactReq q =
      cross_request(hdr, d_subjects, S, d_resources, R, n_contexts, d_out_packed, d_out_errs, err_cap, nullptr);
  REQUIRE(aligned(d_subjects), GCK_E_INVALID_ARGUMENT, "device request: d_subjects is not 4-byte aligned");
  REQUIRE(aligned(d_resources), GCK_E_INVALID_ARGUMENT, "device request: d_resources is not 4-byte aligned");
  return device_request(q, d_out_errs, d_out_n_errs, stream, engine_stream);
}

int gck_check_bulk_cross_device(gck_engine* ge, const gck_consistency* cs, const gck_uniform* hdr,
                                const uint32_t* d_subjects, size_t n_subjects, const uint32_t* d_resources,
                                size_t n_resources, const char* const* contexts, const size_t* context_lens,
                                size_t n_contexts, int64_t now_us, uint64_t* d_out_packed, gck_item_error* d_out_errs,
                                size_t err_cap, uint32_t* d_out_n_errs, void* stream, uint64_t* out_revision) {
  return guard([&] {
    Engine& e = need(ge);
    const CompactReq req = cross_device_request(hdr, d_subjects, n_subjects, d_resources, n_resources, n_contexts,
                                                d_out_packed, d_out_errs, err_cap, d_out_n_errs, stream, true);
    const CallCtx c{cs, contexts, context_lens, n_contexts};
    if (req.n == 0) return check_device_sync(e, c, req, now_us, out_revision);
    // two workspaces when the request is more than one batch either way: more than one tile, or
    // (expanded) more than a chunk
    uint32_t rows = 0;
    const size_t mb = max_batch_of(e);
    const size_t one = gck_cross_tile_device(n_subjects, n_resources, mb, &rows) ? (size_t)rows * n_resources
                                                                                 : (mb & ~(size_t)31);
    check_sync(e, c, req.n, one, out_revision,
               [&](Workspace* w0, Workspace* w1, const CavCall& cav) { device_check_compact(e, w0, w1, req, now_us, cav); });
  });
}

int gck_check_submit_cross_device(gck_engine* ge, const gck_consistency* cs, const gck_uniform* hdr,
                                  const uint32_t* d_subjects, size_t n_subjects, const uint32_t* d_resources,
                                  size_t n_resources, const char* const* contexts, const size_t* context_lens,
                                  size_t n_contexts, int64_t now_us, uint64_t* d_out_packed,
                                  gck_item_error* d_out_errs, size_t err_cap, uint32_t* d_out_n_errs, uint32_t flags,
                                  void* stream, gck_batch** out) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(out, GCK_E_INVALID_ARGUMENT, "null out");
    *out = nullptr;
    check_submit_flags(flags);
    const CompactReq req =
        cross_device_request(hdr, d_subjects, n_subjects, d_resources, n_resources, n_contexts, d_out_packed, d_out_errs,
                             err_cap, d_out_n_errs, stream, (flags & GCK_SUBMIT_ENGINE_STREAM) != 0);
    uint32_t rows = 0;
    REQUIRE(req.n == 0 || (gck_cross_tile_device(n_subjects, n_resources, max_batch_of(e), &rows) && rows == n_subjects),
            GCK_E_INVALID_ARGUMENT,
            "submitted cross device request of " + std::to_string(n_subjects) + " x " + std::to_string(n_resources) +
                " is not one tile (gck_cross_tile_device)");
    *out = submit_device(e, {cs, contexts, context_lens, n_contexts}, req, now_us);
  });
}

// ---- filter requests (include/gck.h gck_filter_list_device) -----------------------------------

// A filter request's selection against the call, before anything is launched; then the list device
// request with it (`sel` is the caller's: the engine copies it per chunk before the call returns).
static CompactReq filter_request(const gck_select* sel, CompactReq q) {
  const auto aligned = [](const void* p) { return ((uintptr_t)p & 3u) == 0; };
  REQUIRE(sel, GCK_E_INVALID_ARGUMENT, "filter request: null gck_select");
  REQUIRE(sel->mask != 0 && !(sel->mask & ~0xEu), GCK_E_INVALID_ARGUMENT,
          "filter request: mask must select among GCK_SELECT_NO, GCK_SELECT_HAS and GCK_SELECT_CONDITIONAL");
  REQUIRE(sel->reserved == 0, GCK_E_INVALID_ARGUMENT, "filter request: gck_select.reserved must be 0");
  REQUIRE(sel->d_out_n, GCK_E_INVALID_ARGUMENT, "filter request: null d_out_n");
  REQUIRE(sel->cap == 0 || sel->d_out_ids || sel->d_out_pos || sel->d_out_perm, GCK_E_INVALID_ARGUMENT,
          "filter request: cap > 0 without an output array");
  REQUIRE(aligned(sel->d_out_ids) && aligned(sel->d_out_pos) && aligned(sel->d_out_n), GCK_E_INVALID_ARGUMENT,
          "filter request: d_out_ids, d_out_pos or d_out_n is not 4-byte aligned");
  q.sel = sel;
  return q;
}

int gck_filter_list_device(gck_engine* ge, const gck_consistency* cs, const gck_uniform* hdr, uint32_t fixed_id,
                           uint32_t vary, const uint32_t* d_ids, uint32_t first_id, size_t n,
                           const char* const* contexts, const size_t* context_lens, size_t n_contexts, int64_t now_us,
                           const gck_select* sel, uint64_t* d_out_packed, gck_item_error* d_out_errs, size_t err_cap,
                           uint32_t* d_out_n_errs, void* stream, uint64_t* out_revision) {
  return guard([&] {
    Engine& e = need(ge);
    const CompactReq req = filter_request(
        sel, device_request(list_request(hdr, fixed_id, vary, d_ids, first_id, n, n_contexts, d_out_packed, d_out_errs,
                                         err_cap, nullptr, false),
                            d_out_errs, d_out_n_errs, stream, true));
    check_device_sync(e, {cs, contexts, context_lens, n_contexts}, req, now_us, out_revision);
  });
}

int gck_filter_submit_list_device(gck_engine* ge, const gck_consistency* cs, const gck_uniform* hdr, uint32_t fixed_id,
                                  uint32_t vary, const uint32_t* d_ids, uint32_t first_id, size_t n,
                                  const char* const* contexts, const size_t* context_lens, size_t n_contexts,
                                  int64_t now_us, const gck_select* sel, uint64_t* d_out_packed,
                                  gck_item_error* d_out_errs, size_t err_cap, uint32_t* d_out_n_errs, uint32_t flags,
                                  void* stream, gck_batch** out) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(out, GCK_E_INVALID_ARGUMENT, "null out");
    *out = nullptr;
    check_submit_flags(flags);
    const CompactReq req = filter_request(
        sel, device_request(list_request(hdr, fixed_id, vary, d_ids, first_id, n, n_contexts, d_out_packed, d_out_errs,
                                         err_cap, nullptr, false),
                            d_out_errs, d_out_n_errs, stream, (flags & GCK_SUBMIT_ENGINE_STREAM) != 0));
    *out = submit_device(e, {cs, contexts, context_lens, n_contexts}, req, now_us);
  });
}

// ---- cross filter requests (include/gck.h gck_filter_cross_device) ----------------------------

// The selection's own argument rules, shared with the host hook (gck_test_select_rows): null when
// the selection is good, else what is wrong with it.
static const char* select_rows_fault(const gck_select_rows* sel) {
  const auto aligned = [](const void* p) { return ((uintptr_t)p & 3u) == 0; };
  if (!sel) return "cross filter request: null gck_select_rows";
  if (sel->mask == 0 || (sel->mask & ~0xEu))
    return "cross filter request: mask must select among GCK_SELECT_NO, GCK_SELECT_HAS and GCK_SELECT_CONDITIONAL";
  if (!sel->d_out_row_off) return "cross filter request: null d_out_row_off";
  if (!sel->d_out_n) return "cross filter request: null d_out_n";
  if (sel->cap != 0 && !sel->d_out_ids && !sel->d_out_col && !sel->d_out_perm)
    return "cross filter request: cap > 0 without an output array";
  if (!aligned(sel->d_out_row_off) || !aligned(sel->d_out_row_n) || !aligned(sel->d_out_ids) ||
      !aligned(sel->d_out_col) || !aligned(sel->d_out_n))
    return "cross filter request: d_out_row_off, d_out_row_n, d_out_ids, d_out_col or d_out_n is not 4-byte aligned";
  return nullptr;
}

// A cross filter request's selection against the call, before anything is launched or written; then
// the cross device request with it (`sel` is the caller's: the engine copies it before the call returns).
static CompactReq filter_cross_request(const gck_select_rows* sel, const gck_uniform* hdr, const uint32_t* d_subjects,
                                       size_t S, const uint32_t* d_resources, size_t R, size_t n_contexts,
                                       uint64_t* d_out_packed, gck_item_error* d_out_errs, size_t err_cap,
                                       uint32_t* d_out_n_errs, void* stream, bool engine_stream) {
  const char* fault = select_rows_fault(sel);
  REQUIRE(!fault, GCK_E_INVALID_ARGUMENT, fault ? fault : "");
  REQUIRE(d_out_packed, GCK_E_INVALID_ARGUMENT, "cross filter request: null d_out_packed");
  CompactReq q = cross_device_request(hdr, d_subjects, S, d_resources, R, n_contexts, d_out_packed, d_out_errs, err_cap,
                                      d_out_n_errs, stream, engine_stream);
  q.sel_rows = sel;
  return q;
}

int gck_filter_cross_device(gck_engine* ge, const gck_consistency* cs, const gck_uniform* hdr,
                            const uint32_t* d_subjects, size_t n_subjects, const uint32_t* d_resources,
                            size_t n_resources, const char* const* contexts, const size_t* context_lens,
                            size_t n_contexts, int64_t now_us, const gck_select_rows* sel, uint64_t* d_out_packed,
                            gck_item_error* d_out_errs, size_t err_cap, uint32_t* d_out_n_errs, void* stream,
                            uint64_t* out_revision) {
  return guard([&] {
    Engine& e = need(ge);
    const CompactReq req = filter_cross_request(sel, hdr, d_subjects, n_subjects, d_resources, n_resources, n_contexts,
                                                d_out_packed, d_out_errs, err_cap, d_out_n_errs, stream, true);
    const CallCtx c{cs, contexts, context_lens, n_contexts};
    if (req.n == 0) {  // (no check runs: the count word, then the offsets and counts of S empty rows)
      check_device_sync(e, c, req, now_us, out_revision);
      return device_select_rows_empty(e, *sel, n_subjects, stream);
    }
    // (the workspaces of gck_check_bulk_cross_device)
    uint32_t rows = 0;
    const size_t mb = max_batch_of(e);
    const size_t one = gck_cross_tile_device(n_subjects, n_resources, mb, &rows) ? (size_t)rows * n_resources
                                                                                 : (mb & ~(size_t)31);
    check_sync(e, c, req.n, one, out_revision,
               [&](Workspace* w0, Workspace* w1, const CavCall& cav) { device_check_compact(e, w0, w1, req, now_us, cav); });
  });
}

int gck_filter_submit_cross_device(gck_engine* ge, const gck_consistency* cs, const gck_uniform* hdr,
                                   const uint32_t* d_subjects, size_t n_subjects, const uint32_t* d_resources,
                                   size_t n_resources, const char* const* contexts, const size_t* context_lens,
                                   size_t n_contexts, int64_t now_us, const gck_select_rows* sel,
                                   uint64_t* d_out_packed, gck_item_error* d_out_errs, size_t err_cap,
                                   uint32_t* d_out_n_errs, uint32_t flags, void* stream, gck_batch** out) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(out, GCK_E_INVALID_ARGUMENT, "null out");
    *out = nullptr;
    check_submit_flags(flags);
    const bool own = (flags & GCK_SUBMIT_ENGINE_STREAM) != 0;
    const CompactReq req = filter_cross_request(sel, hdr, d_subjects, n_subjects, d_resources, n_resources, n_contexts,
                                                d_out_packed, d_out_errs, err_cap, d_out_n_errs, stream, own);
    uint32_t rows = 0;
    REQUIRE(req.n == 0 || (gck_cross_tile_device(n_subjects, n_resources, max_batch_of(e), &rows) && rows == n_subjects),
            GCK_E_INVALID_ARGUMENT,
            "submitted cross filter request of " + std::to_string(n_subjects) + " x " + std::to_string(n_resources) +
                " is not one tile (gck_cross_tile_device)");
    gck_batch* b = submit_device(e, {cs, contexts, context_lens, n_contexts}, req, now_us);
    if (req.n == 0) {
      try {
        device_select_rows_empty(e, *sel, n_subjects, own ? nullptr : stream);
      } catch (...) {
        delete b;
        throw;
      }
    }
    *out = b;
  });
}

// ---- cross filter requests by resource (include/gck.h gck_filter_cross_cols_device) -----------

// The selection's own argument rules, shared with the host hook (gck_test_select_cols): null when
// the selection is good, else what is wrong with it.
static const char* select_cols_fault(const gck_select_cols* sel) {
  const auto aligned = [](const void* p) { return ((uintptr_t)p & 3u) == 0; };
  if (!sel) return "cross filter request by resource: null gck_select_cols";
  if (sel->mask == 0 || (sel->mask & ~0xEu))
    return "cross filter request by resource: mask must select among GCK_SELECT_NO, GCK_SELECT_HAS and "
           "GCK_SELECT_CONDITIONAL";
  if (!sel->d_out_col_off) return "cross filter request by resource: null d_out_col_off";
  if (!sel->d_out_n) return "cross filter request by resource: null d_out_n";
  if (sel->cap != 0 && !sel->d_out_ids && !sel->d_out_row && !sel->d_out_perm)
    return "cross filter request by resource: cap > 0 without an output array";
  if (!aligned(sel->d_out_col_off) || !aligned(sel->d_out_col_n) || !aligned(sel->d_out_ids) ||
      !aligned(sel->d_out_row) || !aligned(sel->d_out_n))
    return "cross filter request by resource: d_out_col_off, d_out_col_n, d_out_ids, d_out_row or d_out_n is not "
           "4-byte aligned";
  return nullptr;
}

// filter_cross_request's twin: the selection against the call, before anything is launched or
// written; then the cross device request with it (`sel` is the caller's: the engine copies it).
static CompactReq filter_cross_cols_request(const gck_select_cols* sel, const gck_uniform* hdr, const uint32_t* d_subjects,
                                            size_t S, const uint32_t* d_resources, size_t R, size_t n_contexts,
                                            uint64_t* d_out_packed, gck_item_error* d_out_errs, size_t err_cap,
                                            uint32_t* d_out_n_errs, void* stream, bool engine_stream) {
  const char* fault = select_cols_fault(sel);
  REQUIRE(!fault, GCK_E_INVALID_ARGUMENT, fault ? fault : "");
  REQUIRE(d_out_packed, GCK_E_INVALID_ARGUMENT, "cross filter request by resource: null d_out_packed");
  CompactReq q = cross_device_request(hdr, d_subjects, S, d_resources, R, n_contexts, d_out_packed, d_out_errs, err_cap,
                                      d_out_n_errs, stream, engine_stream);
  q.sel_cols = sel;
  return q;
}

int gck_filter_cross_cols_device(gck_engine* ge, const gck_consistency* cs, const gck_uniform* hdr,
                                 const uint32_t* d_subjects, size_t n_subjects, const uint32_t* d_resources,
                                 size_t n_resources, const char* const* contexts, const size_t* context_lens,
                                 size_t n_contexts, int64_t now_us, const gck_select_cols* sel,
                                 uint64_t* d_out_packed, gck_item_error* d_out_errs, size_t err_cap,
                                 uint32_t* d_out_n_errs, void* stream, uint64_t* out_revision) {
  return guard([&] {
    Engine& e = need(ge);
    const CompactReq req = filter_cross_cols_request(sel, hdr, d_subjects, n_subjects, d_resources, n_resources,
                                                     n_contexts, d_out_packed, d_out_errs, err_cap, d_out_n_errs, stream,
                                                     true);
    const CallCtx c{cs, contexts, context_lens, n_contexts};
    if (req.n == 0) {  // (no check runs: the count word, then the offsets and counts of R empty columns)
      check_device_sync(e, c, req, now_us, out_revision);
      return device_select_cols_empty(e, *sel, n_resources, stream);
    }
    // (the workspaces of gck_check_bulk_cross_device)
    uint32_t rows = 0;
    const size_t mb = max_batch_of(e);
    const size_t one = gck_cross_tile_device(n_subjects, n_resources, mb, &rows) ? (size_t)rows * n_resources
                                                                                 : (mb & ~(size_t)31);
    check_sync(e, c, req.n, one, out_revision,
               [&](Workspace* w0, Workspace* w1, const CavCall& cav) { device_check_compact(e, w0, w1, req, now_us, cav); });
  });
}

int gck_filter_submit_cross_cols_device(gck_engine* ge, const gck_consistency* cs, const gck_uniform* hdr,
                                        const uint32_t* d_subjects, size_t n_subjects, const uint32_t* d_resources,
                                        size_t n_resources, const char* const* contexts, const size_t* context_lens,
                                        size_t n_contexts, int64_t now_us, const gck_select_cols* sel,
                                        uint64_t* d_out_packed, gck_item_error* d_out_errs, size_t err_cap,
                                        uint32_t* d_out_n_errs, uint32_t flags, void* stream, gck_batch** out) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(out, GCK_E_INVALID_ARGUMENT, "null out");
    *out = nullptr;
    check_submit_flags(flags);
    const bool own = (flags & GCK_SUBMIT_ENGINE_STREAM) != 0;
    const CompactReq req = filter_cross_cols_request(sel, hdr, d_subjects, n_subjects, d_resources, n_resources,
                                                     n_contexts, d_out_packed, d_out_errs, err_cap, d_out_n_errs, stream,
                                                     own);
    uint32_t rows = 0;
    REQUIRE(req.n == 0 || (gck_cross_tile_device(n_subjects, n_resources, max_batch_of(e), &rows) && rows == n_subjects),
            GCK_E_INVALID_ARGUMENT,
            "submitted cross filter request by resource of " + std::to_string(n_subjects) + " x " +
                std::to_string(n_resources) + " is not one tile (gck_cross_tile_device)");
    gck_batch* b = submit_device(e, {cs, contexts, context_lens, n_contexts}, req, now_us);
    if (req.n == 0) {
      try {
        device_select_cols_empty(e, *sel, n_resources, own ? nullptr : stream);
      } catch (...) {
        delete b;
        throw;
      }
    }
    *out = b;
  });
}

// ---- group filter requests (include/gck.h gck_filter_groups_device) ---------------------------

// The request's argument rules, every one of them, shared with the host hook (gck_test_groups_rule):
// empty when the request is good, else what is wrong with it. Reads no buffer but *hdr and *sel.
static std::string groups_fault(const gck_uniform* hdr, uint32_t vary, const uint32_t* d_owners, size_t S,
                                const uint32_t* d_group_off, const uint32_t* d_candidates, size_t n, size_t n_contexts,
                                const gck_select_groups* sel, const uint64_t* d_out_packed, const gck_item_error* d_out_errs,
                                size_t err_cap, const uint32_t* d_out_n_errs) {
  const auto aligned = [](const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; };
  const std::string g = "group filter request: ";
  if (!hdr) return "null header";
  if (hdr->context_slot > n_contexts)
    return "uniform header: context_slot " + std::to_string(hdr->context_slot) + " beyond the " + std::to_string(n_contexts) +
           " contexts given";
  if (hdr->reserved != 0) return g + "the header's reserved must be 0";
  if (vary != GCK_VARY_RESOURCE && vary != GCK_VARY_SUBJECT) return g + "vary must be GCK_VARY_RESOURCE or GCK_VARY_SUBJECT";
  if (!sel) return g + "null gck_select_groups";
  if (sel->mask == 0 || (sel->mask & ~0xEu))
    return g + "mask must select among GCK_SELECT_NO, GCK_SELECT_HAS and GCK_SELECT_CONDITIONAL";
  if (!sel->d_out_row_off) return g + "null d_out_row_off";
  if (!sel->d_out_n) return g + "null d_out_n";
  if (!d_out_packed) return g + "null d_out_packed";
  if (sel->cap != 0 && !sel->d_out_ids && !sel->d_out_pos && !sel->d_out_perm) return g + "cap > 0 without an output array";
  if (n >= 0x100000000ull) return g + std::to_string(n) + " checks reach 2^32";
  if (S >= 0x100000000ull) return g + std::to_string(S) + " groups reach 2^32";
  if (n > 0 && S == 0) return g + std::to_string(n) + " candidates without a group";
  if (n > 0 && (!d_owners || !d_group_off || !d_candidates)) return g + "null d_owners, d_group_off or d_candidates";
  if (err_cap != 0 && !d_out_errs) return "null error list";
  if (!aligned(d_out_packed, 8)) return g + "d_out_packed is not 8-byte aligned";
  if (!aligned(d_owners, 4) || !aligned(d_group_off, 4) || !aligned(d_candidates, 4))
    return g + "d_owners, d_group_off or d_candidates is not 4-byte aligned";
  if (!aligned(d_out_errs, 4) || !aligned(d_out_n_errs, 4)) return g + "d_out_errs or d_out_n_errs is not 4-byte aligned";
  if (!aligned(sel->d_out_row_off, 4) || !aligned(sel->d_out_row_n, 4) || !aligned(sel->d_out_ids, 4) ||
      !aligned(sel->d_out_pos, 4) || !aligned(sel->d_out_n, 4))
    return g + "d_out_row_off, d_out_row_n, d_out_ids, d_out_pos or d_out_n is not 4-byte aligned";
  return std::string();
}

// The rules against the call, before anything is launched or written; then the request as the engine
// takes it (`sel` is the caller's: the engine copies it before the call returns).
static CompactReq groups_request(const gck_uniform* hdr, uint32_t vary, const uint32_t* d_owners, size_t S,
                                 const uint32_t* d_group_off, const uint32_t* d_candidates, size_t n, size_t n_contexts,
                                 const gck_select_groups* sel, uint64_t* d_out_packed, gck_item_error* d_out_errs,
                                 size_t err_cap, uint32_t* d_out_n_errs, void* stream, bool engine_stream) {
  const std::string fault = groups_fault(hdr, vary, d_owners, S, d_group_off, d_candidates, n, n_contexts, sel, d_out_packed,
                                         d_out_errs, err_cap, d_out_n_errs);
  REQUIRE(fault.empty(), GCK_E_INVALID_ARGUMENT, fault);
  CompactReq q{hdr, 1u, nullptr, nullptr, n, d_out_packed, d_out_errs, err_cap, nullptr};
  q.vary = vary;
  q.ids = d_candidates;
  q.owners = d_owners;
  q.group_off = d_group_off;
  q.S = S;
  q.sel_groups = sel;
  q.device = true;
  q.engine_stream = engine_stream;
  q.stream = stream;
  q.d_n_errs = d_out_n_errs;
  return q;
}

int gck_filter_groups_device(gck_engine* ge, const gck_consistency* cs, const gck_uniform* hdr, uint32_t vary,
                             const uint32_t* d_owners, size_t n_owners, const uint32_t* d_group_off,
                             const uint32_t* d_candidates, size_t n_candidates, const char* const* contexts,
                             const size_t* context_lens, size_t n_contexts, int64_t now_us,
                             const gck_select_groups* sel, uint64_t* d_out_packed, gck_item_error* d_out_errs,
                             size_t err_cap, uint32_t* d_out_n_errs, void* stream, uint64_t* out_revision) {
  return guard([&] {
    Engine& e = need(ge);
    const CompactReq req = groups_request(hdr, vary, d_owners, n_owners, d_group_off, d_candidates, n_candidates, n_contexts,
                                          sel, d_out_packed, d_out_errs, err_cap, d_out_n_errs, stream, true);
    const CallCtx c{cs, contexts, context_lens, n_contexts};
    check_device_sync(e, c, req, now_us, out_revision);
    // (no check ran: the count word above, then the offsets and counts of S empty groups)
    if (req.n == 0) device_select_groups_empty(e, *sel, n_owners, stream);
  });
}

int gck_filter_submit_groups_device(gck_engine* ge, const gck_consistency* cs, const gck_uniform* hdr, uint32_t vary,
                                    const uint32_t* d_owners, size_t n_owners, const uint32_t* d_group_off,
                                    const uint32_t* d_candidates, size_t n_candidates, const char* const* contexts,
                                    const size_t* context_lens, size_t n_contexts, int64_t now_us,
                                    const gck_select_groups* sel, uint64_t* d_out_packed, gck_item_error* d_out_errs,
                                    size_t err_cap, uint32_t* d_out_n_errs, uint32_t flags, void* stream,
                                    gck_batch** out) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(out, GCK_E_INVALID_ARGUMENT, "null out");
    *out = nullptr;
    check_submit_flags(flags);
    const bool own = (flags & GCK_SUBMIT_ENGINE_STREAM) != 0;
    const CompactReq req = groups_request(hdr, vary, d_owners, n_owners, d_group_off, d_candidates, n_candidates, n_contexts,
                                          sel, d_out_packed, d_out_errs, err_cap, d_out_n_errs, stream, own);
    REQUIRE(req.n <= max_batch_of(e), GCK_E_INVALID_ARGUMENT,
            "submitted group filter request of " + std::to_string(req.n) + " checks is above max_batch");
    gck_batch* b = submit_device(e, {cs, contexts, context_lens, n_contexts}, req, now_us);
    if (req.n == 0) {
      try {
        device_select_groups_empty(e, *sel, n_owners, own ? nullptr : stream);
      } catch (...) {
        delete b;
        throw;
      }
    }
    *out = b;
  });
}

// ---- recheck requests (include/gck.h gck_recheck_list_device) ---------------------------------

// The rules of the two forms beyond the underlying call's own, each in one function shared by the
// form's entry points, its plane-only call and the host hooks (gck_test_changes_rule,
// gck_test_row_changes_rule): empty when the arguments are good, else what is wrong with them. Reads
// no buffer but *sel. `words`: the 8-B words of each plane; need_plane: the new plane is required.
static std::string change_common_fault(const std::string& g, uint32_t transitions, uint32_t reserved, const void* d_out_n,
                                       bool arrays, size_t cap, const uint64_t* d_prev, const uint64_t* d_out,
                                       size_t words, bool need_plane) {
  const auto aligned = [](const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; };
  if (transitions == 0 || (transitions & ~(uint32_t)GCK_CHANGE_ANY))
    return g + "transitions must be non-zero and within GCK_CHANGE_ANY";
  if (reserved != 0) return g + "reserved must be 0";
  if (!d_out_n) return g + "null d_out_n";
  if (need_plane && !d_out) return g + "null d_out_packed";
  if (cap != 0 && !arrays) return g + "cap > 0 without an output array";
  if (!aligned(d_prev, 8) || !aligned(d_out, 8)) return g + "d_prev_packed or d_out_packed is not 8-byte aligned";
  if (d_prev && d_out && words) {
    const uintptr_t a = (uintptr_t)d_prev, b = (uintptr_t)d_out, len = (uintptr_t)words * 8u;
    if (a < b + len && b < a + len) return g + "d_prev_packed overlaps d_out_packed";
  }
  return std::string();
}

static std::string changes_fault(const gck_select_changes* sel, const uint64_t* d_prev, const uint64_t* d_out, size_t n,
                                 bool need_plane) {
  const auto aligned = [](const void* p) { return ((uintptr_t)p & 3u) == 0; };
  const std::string g = "recheck request: ";
  if (!sel) return g + "null gck_select_changes";
  const std::string f =
      change_common_fault(g, sel->transitions, sel->reserved, sel->d_out_n, sel->d_out_ids || sel->d_out_pos || sel->d_out_trans,
                          sel->cap, d_prev, d_out, n / 32u + (n % 32u != 0), need_plane);
  if (!f.empty()) return f;
  if (!aligned(sel->d_out_ids) || !aligned(sel->d_out_pos) || !aligned(sel->d_out_n))
    return g + "d_out_ids, d_out_pos or d_out_n is not 4-byte aligned";
  return std::string();
}

static std::string row_changes_fault(const gck_select_row_changes* sel, const uint64_t* d_prev, const uint64_t* d_out,
                                     size_t S, size_t R, bool need_plane) {
  const auto aligned = [](const void* p) { return ((uintptr_t)p & 3u) == 0; };
  const std::string g = "recheck cross request: ";
  if (!sel) return g + "null gck_select_row_changes";
  if (!sel->d_out_row_off) return g + "null d_out_row_off";
  const size_t stride = R / 32u + (R % 32u != 0);
  if (stride && S > SIZE_MAX / 8u / stride) return g + "the plane is too large";
  const std::string f =
      change_common_fault(g, sel->transitions, sel->reserved, sel->d_out_n, sel->d_out_ids || sel->d_out_col || sel->d_out_trans,
                          sel->cap, d_prev, d_out, S * stride, need_plane);
  if (!f.empty()) return f;
  if (!aligned(sel->d_out_row_off) || !aligned(sel->d_out_ids) || !aligned(sel->d_out_col) || !aligned(sel->d_out_n))
    return g + "d_out_row_off, d_out_ids, d_out_col or d_out_n is not 4-byte aligned";
  return std::string();
}

// The rules against the call, before anything is launched or written; then the list device request
// with the diff (`sel` is the caller's: the engine copies it before the call returns).
static CompactReq recheck_list_request(const uint64_t* d_prev, const gck_select_changes* sel, const gck_uniform* hdr,
                                       uint32_t fixed_id, uint32_t vary, const uint32_t* d_ids, uint32_t first_id, size_t n,
                                       size_t n_contexts, uint64_t* d_out_packed, gck_item_error* d_out_errs, size_t err_cap,
                                       uint32_t* d_out_n_errs, void* stream, bool engine_stream) {
  const std::string fault = changes_fault(sel, d_prev, d_out_packed, n, true);
  REQUIRE(fault.empty(), GCK_E_INVALID_ARGUMENT, fault);
  CompactReq q = device_request(
      list_request(hdr, fixed_id, vary, d_ids, first_id, n, n_contexts, d_out_packed, d_out_errs, err_cap, nullptr),
      d_out_errs, d_out_n_errs, stream, engine_stream);
  q.prev = d_prev;
  q.diff = sel;
  return q;
}

int gck_recheck_list_device(gck_engine* ge, const gck_consistency* cs, const gck_uniform* hdr, uint32_t fixed_id,
                            uint32_t vary, const uint32_t* d_ids, uint32_t first_id, size_t n,
                            const char* const* contexts, const size_t* context_lens, size_t n_contexts, int64_t now_us,
                            const uint64_t* d_prev_packed, const gck_select_changes* sel, uint64_t* d_out_packed,
                            gck_item_error* d_out_errs, size_t err_cap, uint32_t* d_out_n_errs, void* stream,
                            uint64_t* out_revision) {
  return guard([&] {
    Engine& e = need(ge);
    const CompactReq req = recheck_list_request(d_prev_packed, sel, hdr, fixed_id, vary, d_ids, first_id, n, n_contexts,
                                                d_out_packed, d_out_errs, err_cap, d_out_n_errs, stream, true);
    check_device_sync(e, {cs, contexts, context_lens, n_contexts}, req, now_us, out_revision);
    if (req.n == 0) device_zero_count(e, sel->d_out_n, stream);  // (no check ran: no change)
  });
}

int gck_recheck_submit_list_device(gck_engine* ge, const gck_consistency* cs, const gck_uniform* hdr, uint32_t fixed_id,
                                   uint32_t vary, const uint32_t* d_ids, uint32_t first_id, size_t n,
                                   const char* const* contexts, const size_t* context_lens, size_t n_contexts,
                                   int64_t now_us, const uint64_t* d_prev_packed, const gck_select_changes* sel,
                                   uint64_t* d_out_packed, gck_item_error* d_out_errs, size_t err_cap,
                                   uint32_t* d_out_n_errs, uint32_t flags, void* stream, gck_batch** out) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(out, GCK_E_INVALID_ARGUMENT, "null out");
    *out = nullptr;
    check_submit_flags(flags);
    const bool own = (flags & GCK_SUBMIT_ENGINE_STREAM) != 0;
    const CompactReq req = recheck_list_request(d_prev_packed, sel, hdr, fixed_id, vary, d_ids, first_id, n, n_contexts,
                                                d_out_packed, d_out_errs, err_cap, d_out_n_errs, stream, own);
    gck_batch* b = submit_device(e, {cs, contexts, context_lens, n_contexts}, req, now_us);
    if (req.n == 0) {
      try {
        device_zero_count(e, sel->d_out_n, own ? nullptr : stream);
      } catch (...) {
        delete b;
        throw;
      }
    }
    *out = b;
  });
}

static CompactReq recheck_cross_request(const uint64_t* d_prev, const gck_select_row_changes* sel, const gck_uniform* hdr,
                                        const uint32_t* d_subjects, size_t S, const uint32_t* d_resources, size_t R,
                                        size_t n_contexts, uint64_t* d_out_packed, gck_item_error* d_out_errs,
                                        size_t err_cap, uint32_t* d_out_n_errs, void* stream, bool engine_stream) {
  const std::string fault = row_changes_fault(sel, d_prev, d_out_packed, S, R, true);
  REQUIRE(fault.empty(), GCK_E_INVALID_ARGUMENT, fault);
  CompactReq q = cross_device_request(hdr, d_subjects, S, d_resources, R, n_contexts, d_out_packed, d_out_errs, err_cap,
                                      d_out_n_errs, stream, engine_stream);
  q.prev = d_prev;
  q.diff_rows = sel;
  return q;
}

int gck_recheck_cross_device(gck_engine* ge, const gck_consistency* cs, const gck_uniform* hdr,
                             const uint32_t* d_subjects, size_t n_subjects, const uint32_t* d_resources,
                             size_t n_resources, const char* const* contexts, const size_t* context_lens,
                             size_t n_contexts, int64_t now_us, const uint64_t* d_prev_packed,
                             const gck_select_row_changes* sel, uint64_t* d_out_packed, gck_item_error* d_out_errs,
                             size_t err_cap, uint32_t* d_out_n_errs, void* stream, uint64_t* out_revision) {
  return guard([&] {
    Engine& e = need(ge);
    const CompactReq req = recheck_cross_request(d_prev_packed, sel, hdr, d_subjects, n_subjects, d_resources, n_resources,
                                                 n_contexts, d_out_packed, d_out_errs, err_cap, d_out_n_errs, stream, true);
    const CallCtx c{cs, contexts, context_lens, n_contexts};
    if (req.n == 0) {  // (no check runs: the count word, then the offsets of S rows without a change)
      check_device_sync(e, c, req, now_us, out_revision);
      return device_diff_rows(e, *sel, nullptr, nullptr, n_subjects, n_resources, nullptr, stream);
    }
    // (the workspaces of gck_check_bulk_cross_device)
    uint32_t rows = 0;
    const size_t mb = max_batch_of(e);
    const size_t one = gck_cross_tile_device(n_subjects, n_resources, mb, &rows) ? (size_t)rows * n_resources
                                                                                 : (mb & ~(size_t)31);
    check_sync(e, c, req.n, one, out_revision,
               [&](Workspace* w0, Workspace* w1, const CavCall& cav) { device_check_compact(e, w0, w1, req, now_us, cav); });
  });
}

int gck_recheck_submit_cross_device(gck_engine* ge, const gck_consistency* cs, const gck_uniform* hdr,
                                    const uint32_t* d_subjects, size_t n_subjects, const uint32_t* d_resources,
                                    size_t n_resources, const char* const* contexts, const size_t* context_lens,
                                    size_t n_contexts, int64_t now_us, const uint64_t* d_prev_packed,
                                    const gck_select_row_changes* sel, uint64_t* d_out_packed,
                                    gck_item_error* d_out_errs, size_t err_cap, uint32_t* d_out_n_errs, uint32_t flags,
                                    void* stream, gck_batch** out) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(out, GCK_E_INVALID_ARGUMENT, "null out");
    *out = nullptr;
    check_submit_flags(flags);
    const bool own = (flags & GCK_SUBMIT_ENGINE_STREAM) != 0;
    const CompactReq req = recheck_cross_request(d_prev_packed, sel, hdr, d_subjects, n_subjects, d_resources, n_resources,
                                                 n_contexts, d_out_packed, d_out_errs, err_cap, d_out_n_errs, stream, own);
    uint32_t rows = 0;
    REQUIRE(req.n == 0 || (gck_cross_tile_device(n_subjects, n_resources, max_batch_of(e), &rows) && rows == n_subjects),
            GCK_E_INVALID_ARGUMENT,
            "submitted recheck cross request of " + std::to_string(n_subjects) + " x " + std::to_string(n_resources) +
                " is not one tile (gck_cross_tile_device)");
    gck_batch* b = submit_device(e, {cs, contexts, context_lens, n_contexts}, req, now_us);
    if (req.n == 0) {
      try {
        device_diff_rows(e, *sel, nullptr, nullptr, n_subjects, n_resources, nullptr, own ? nullptr : stream);
      } catch (...) {
        delete b;
        throw;
      }
    }
    *out = b;
  });
}

// The plane-only calls: the selection alone over two planes the caller holds.
int gck_diff_planes_device(gck_engine* ge, const uint64_t* d_old, const uint64_t* d_new, size_t n, const uint32_t* d_ids,
                           uint32_t first_id, const gck_select_changes* sel, void* stream) {
  return guard([&] {
    Engine& e = need(ge);
    const std::string fault = changes_fault(sel, d_old, d_new, n, n != 0);
    REQUIRE(fault.empty(), GCK_E_INVALID_ARGUMENT, fault);
    REQUIRE(n < 0x100000000ull, GCK_E_INVALID_ARGUMENT, "recheck request: " + std::to_string(n) + " checks reach 2^32");
    REQUIRE(((uintptr_t)d_ids & 3u) == 0, GCK_E_INVALID_ARGUMENT, "recheck request: d_ids is not 4-byte aligned");
    REQUIRE(d_ids || (uint64_t)first_id + n <= 0x100000000ull, GCK_E_INVALID_ARGUMENT,
            "recheck request: the range " + std::to_string(first_id) + " + " + std::to_string(n) + " passes 2^32");
    precheck(e);
    WsLease lease(e);  // (its pair of count words chains a plane of more than one chunk)
    device_diff_planes(e, *lease.w, *sel, d_old, d_new, n, d_ids, first_id, stream);
  });
}

int gck_diff_cross_planes_device(gck_engine* ge, const uint64_t* d_old, const uint64_t* d_new, size_t n_subjects,
                                 size_t n_resources, const uint32_t* d_resources, const gck_select_row_changes* sel,
                                 void* stream) {
  return guard([&] {
    Engine& e = need(ge);
    const bool checks = n_subjects != 0 && n_resources != 0;
    const std::string fault = row_changes_fault(sel, d_old, d_new, n_subjects, n_resources, checks);
    REQUIRE(fault.empty(), GCK_E_INVALID_ARGUMENT, fault);
    REQUIRE(n_subjects < 0x100000000ull && n_resources < 0x100000000ull &&
                (!checks || n_subjects <= 0xFFFFFFFFull / n_resources),
            GCK_E_INVALID_ARGUMENT, "recheck cross request: the checks reach 2^32");
    REQUIRE(((uintptr_t)d_resources & 3u) == 0, GCK_E_INVALID_ARGUMENT, "recheck cross request: d_resources is not 4-byte aligned");
    REQUIRE(!checks || !sel->d_out_ids || d_resources, GCK_E_INVALID_ARGUMENT,
            "recheck cross request: d_out_ids without d_resources");
    precheck(e);
    device_diff_rows(e, *sel, d_old, d_new, n_subjects, n_resources, d_resources, stream);
  });
}

int gck_device_compact_stats(gck_engine* ge, uint64_t out[2]) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(out, GCK_E_INVALID_ARGUMENT, "null out");
    out[0] = e.dev_in_place.load(std::memory_order_relaxed);
    out[1] = e.dev_expanded.load(std::memory_order_relaxed);
  });
}

int gck_host_alloc(gck_engine* ge, size_t bytes, void** out) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(out, GCK_E_INVALID_ARGUMENT, "null out");
    *out = host_alloc(e, bytes);
  });
}

int gck_host_free(gck_engine* ge, void* p) {
  return guard([&] {
    Engine& e = need(ge);
    if (p) host_free(e, p);
  });
}

int gck_check_wait(gck_engine* ge, gck_batch* b) { return gck_check_wait_at(ge, b, nullptr); }

int gck_check_wait_at(gck_engine* ge, gck_batch* b, uint64_t* out_revision) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(b, GCK_E_INVALID_ARGUMENT, "null batch");
    std::unique_ptr<gck_batch> own(b);
    if (out_revision) *out_revision = b->revision;
    if (!b->w) return;
    Workspace* w = b->w;
    try {
      device_wait(e, w);
    } catch (...) {
      release_ws(e, w);
      throw;
    }
    release_ws(e, w);
  });
}

int gck_set_partition(gck_engine* ge, uint32_t rank, uint32_t world) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(world >= 1 && world <= 63 && rank < world, GCK_E_INVALID_ARGUMENT, "bad rank / world");
    WriterLock lk(e);
    REQUIRE(!e.committed && !e.dev && e.ws_pool.empty() && !e.part_ws && e.staged.empty() && e.prebuilt.empty(),
            GCK_E_STATE, "gck_set_partition must precede the first snapshot");
    e.part_rank = rank;
    e.part_world = world;
    e.part_set = true;
    ++e.shape_gen;
    partition_rules(e);
    // the bundles and the bidirectional search need the whole graph; the membership indexes serve
    // the bundles: a partitioned rank's checks are decided by the partitioned label join from the
    // slots, and its level loop (what the join leaves) finds a subject in a row by binary search —
    // at 1e9 tuples the index of the kept memberships alone would be 13 of a rank's 29 GB
    if (world > 1) e.cfg.flags |= GCK_FLAG_NO_BUNDLE | GCK_FLAG_NO_BIDIR | GCK_FLAG_NO_MHASH;
  });
}

uint32_t gck_partition_owner_name(uint16_t type, const char* name, size_t len, uint32_t world) {
  return part_owner_name(type, name ? name : "", name ? len : 0, world);
}

int gck_part_intern_with(gck_engine* ge, const gck_transport* t, const uint16_t* types, const char* const* names,
                         const uint32_t* lens, size_t n, uint32_t flags, uint32_t* out_ids) {
  return guard([&] {
    Engine& e = need(ge);
    need_schema(e);
    REQUIRE(t, GCK_E_INVALID_ARGUMENT, "null transport");
    REQUIRE(n == 0 || (types && names && lens && out_ids), GCK_E_INVALID_ARGUMENT, "null argument");
    WriterLock lk(e);  // (the interner changes; every rank's call blocks in the exchange together)
    part_intern(e, *t, types, names, lens, n, (flags & GCK_INTERN_CREATE) != 0, out_ids);
  });
}

int gck_part_add_tuples_text_with(gck_engine* ge, const gck_transport* t, const char* text, size_t len) {
  return guard([&] {
    Engine& e = need(ge);
    need_schema(e);
    REQUIRE(t, GCK_E_INVALID_ARGUMENT, "null transport");
    REQUIRE(text || !len, GCK_E_INVALID_ARGUMENT, "null text");
    WriterLock lk(e);
    REQUIRE(e.staging, GCK_E_STATE, "gck_begin_snapshot first");
    part_add_tuples_text(e, *t, text, len);
  });
}

int gck_interned_names(gck_engine* ge, uint16_t type, uint32_t* out) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(out, GCK_E_INVALID_ARGUMENT, "null out");
    REQUIRE(type < need_schema(e).types.size(), GCK_E_INVALID_ARGUMENT, "bad type");
    std::shared_lock<std::shared_mutex> lk(e.mu);
    *out = (uint32_t)e.interner[type].ids.size();
  });
}

uint32_t gck_partition_owner(uint32_t object_id, uint32_t world) {
  return world <= 1 ? 0u : part_owner(object_id, world);
}

int gck_part_unique_id(uint8_t* out) {
  return guard([&] {
    REQUIRE(out, GCK_E_INVALID_ARGUMENT, "null id buffer");
    part_unique_id(out);
  });
}

int gck_part_init(gck_engine* ge, const uint8_t* id) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(id, GCK_E_INVALID_ARGUMENT, "null id");
    WriterLock lk(e);
    part_init(e, id);
  });
}

int gck_part_check(gck_engine* ge, const gck_item* d_items, size_t n, int64_t now_us, uint8_t* d_out_perm,
                   int32_t* d_out_err, void* stream) {
  return guard([&] {
    Engine& e = need(ge);
    std::shared_lock<std::shared_mutex> lk(e.mu);
    REQUIRE(e.committed, GCK_E_STATE, "no snapshot committed");
    REQUIRE(n == 0 || (d_items && d_out_perm && d_out_err), GCK_E_INVALID_ARGUMENT, "null buffers");
    part_check(e, d_items, n, now_us, d_out_perm, d_out_err, stream);
  });
}

int gck_part_check_with(gck_engine* ge, const gck_transport* t, const gck_item* d_items, size_t n, int64_t now_us,
                        uint8_t* d_out_perm, int32_t* d_out_err, void* stream) {
  return guard([&] {
    Engine& e = need(ge);
    std::shared_lock<std::shared_mutex> lk(e.mu);
    REQUIRE(e.committed, GCK_E_STATE, "no snapshot committed");
    REQUIRE(t, GCK_E_INVALID_ARGUMENT, "null transport");
    REQUIRE(n == 0 || (d_items && d_out_perm && d_out_err), GCK_E_INVALID_ARGUMENT, "null buffers");
    part_check_with(e, *t, d_items, n, now_us, d_out_perm, d_out_err, stream);
  });
}

// The result of a lookup that did not fit the caller's buffer, kept per thread so that the retry
// with cap >= *out_n copies it out without a second sweep. It matches only a retry of the same
// request on the same snapshot (process-wide snapshot generation) at the same explicit now_us
// (now_us = 0, the wall clock, never matches), and is dropped once copied out.
struct LookupCache {
  uint64_t generation = 0;  // 0 = empty
  gck_item proto{};
  bool vary_res = false;
  int64_t now_us = 0;
  std::vector<uint32_t> ids;
  std::vector<uint8_t> perms;
  // a lookup among candidates (lookup_among): 1 with the caller's list `cand`, 2 over the whole type
  int among = 0;
  std::vector<uint32_t> cand;
};
thread_local LookupCache g_lookup;

// What every lookup checks under the shared engine lock: the engine's state, the consistency asked
// for, and the request's types and relations against the schema.
static void lookup_checks(Engine& e, const gck_consistency* cs, const gck_item& proto) {
  REQUIRE(e.committed, GCK_E_STATE, "no snapshot committed");
  REQUIRE(e.part_world <= 1, GCK_E_STATE, "lookups are not available on a partitioned engine");
  check_consistency(e, cs);
  const Schema& sc = *e.schema;
  REQUIRE(proto.resource_type < sc.types.size() && proto.subject_type < sc.types.size(), GCK_E_NOT_FOUND,
          "object definition not found");
  REQUIRE(proto.permission < sc.rels.size() && sc.rels[proto.permission].type == proto.resource_type,
          GCK_E_NOT_FOUND, "relation/permission not found");
  REQUIRE(proto.subject_relation == GCK_ELLIPSIS ||
              (proto.subject_relation < sc.rels.size() && sc.rels[proto.subject_relation].type == proto.subject_type),
          GCK_E_NOT_FOUND, "subject relation not found");
}

// The end of every lookup: the count, then the kept result (g_lookup) copied out and dropped — or,
// when it exceeds `cap`, kept for the retry and GCK_E_CAPACITY.
static void lookup_copy_out(uint32_t* out_ids, uint8_t* out_perm, size_t cap, size_t* out_n) {
  *out_n = g_lookup.ids.size();
  REQUIRE(cap >= g_lookup.ids.size(), GCK_E_CAPACITY,
          "lookup result has " + std::to_string(g_lookup.ids.size()) + " ids: retry with that capacity");
  if (!g_lookup.ids.empty()) {
    std::memcpy(out_ids, g_lookup.ids.data(), g_lookup.ids.size() * 4);
    std::memcpy(out_perm, g_lookup.perms.data(), g_lookup.perms.size());
  }
  g_lookup.generation = 0;
  g_lookup.ids.clear();
  g_lookup.perms.clear();
  g_lookup.cand.clear();
}

// Whether the kept result answers this request (the candidates apart: lookup_among), and the request
// remembered beside a result just computed.
static bool lookup_kept(const Engine& e, const gck_item& proto, bool vary_res, int64_t now_us, int among) {
  return now_us != 0 && g_lookup.generation != 0 && g_lookup.generation == e.generation && g_lookup.among == among &&
         g_lookup.vary_res == vary_res && g_lookup.now_us == now_us &&
         std::memcmp(&g_lookup.proto, &proto, sizeof(gck_item)) == 0;
}
static void lookup_keep(const Engine& e, const gck_item& proto, bool vary_res, int64_t now_us, int among) {
  g_lookup.generation = e.generation;
  g_lookup.proto = proto;
  g_lookup.vary_res = vary_res;
  g_lookup.now_us = now_us;
  g_lookup.among = among;
  g_lookup.cand.clear();
}

static void lookup(gck_engine* ge, const gck_consistency* cs, const gck_item& proto, bool vary_res, int64_t now_us,
                   uint32_t* out_ids, uint8_t* out_perm, size_t cap, size_t* out_n) {
  Engine& e = need(ge);
  REQUIRE(out_n && (cap == 0 || (out_ids && out_perm)), GCK_E_INVALID_ARGUMENT, "null buffers");
  {
    std::shared_lock<std::shared_mutex> lk(e.mu);
    REQUIRE(e.committed, GCK_E_STATE, "no snapshot committed");
    REQUIRE(e.part_world <= 1, GCK_E_STATE, "lookups are not available on a partitioned engine");
  }
  WsLease lease(e);  // before the engine lock (engine.hpp WsLease)
  std::shared_lock<std::shared_mutex> lk(e.mu);
  lookup_checks(e, cs, proto);
  if (!lookup_kept(e, proto, vary_res, now_us, 0)) {
    g_lookup.generation = 0;
    if (vary_res) {
      device_lookup(e, *lease.w, proto, true, e.interner[proto.resource_type].count, now_us, g_lookup.ids,
                    g_lookup.perms);
    } else {
      device_lookup_subjects(e, *lease.w, proto, now_us, g_lookup.ids, g_lookup.perms);
    }
    lookup_keep(e, proto, vary_res, now_us, 0);
  }
  lookup_copy_out(out_ids, out_perm, cap, out_n);
}

int gck_lookup_resources(gck_engine* ge, const gck_consistency* cs, uint16_t resource_type, uint16_t permission,
                         uint16_t subject_type, uint16_t subject_relation, uint32_t subject_id, int64_t now_us,
                         uint32_t* out_ids, uint8_t* out_perm, size_t cap, size_t* out_n) {
  return guard([&] {
    REQUIRE(subject_id != GCK_ID_WILDCARD, GCK_E_INVALID_ARGUMENT, "cannot perform lookup on wildcard subject");
    gck_item proto{resource_type, permission, 0, subject_type, subject_relation, subject_id, 0};
    lookup(ge, cs, proto, true, now_us, out_ids, out_perm, cap, out_n);
  });
}

int gck_lookup_subjects(gck_engine* ge, const gck_consistency* cs, uint16_t resource_type, uint32_t resource_id,
                        uint16_t permission, uint16_t subject_type, uint16_t subject_relation, int64_t now_us,
                        uint32_t* out_ids, uint8_t* out_perm, size_t cap, size_t* out_n) {
  return guard([&] {
    gck_item proto{resource_type, permission, resource_id, subject_type, subject_relation, 0, 0};
    lookup(ge, cs, proto, false, now_us, out_ids, out_perm, cap, out_n);
  });
}

// gck_lookup_resources_among / gck_lookup_subjects_among: the candidates (null: every object of the
// resource type, one range) as one list request (engine.hpp device_lookup_among), under `lookup`'s
// argument checks and its capacity protocol — the kept result also remembers the candidates.
static void lookup_among(gck_engine* ge, const gck_consistency* cs, const gck_item& proto, bool vary_res,
                         const uint32_t* candidates, size_t n_candidates, int64_t now_us, uint32_t* out_ids,
                         uint8_t* out_perm, size_t cap, size_t* out_n) {
  Engine& e = need(ge);
  REQUIRE(out_n && (cap == 0 || (out_ids && out_perm)), GCK_E_INVALID_ARGUMENT, "null buffers");
  REQUIRE(vary_res || candidates || n_candidates == 0, GCK_E_INVALID_ARGUMENT,
          "lookup among subjects needs a candidate list");
  REQUIRE(n_candidates <= 0xFFFFFFFFull, GCK_E_INVALID_ARGUMENT, "too many candidates");
  precheck(e);
  WsPair p(e, 2);  // before the engine lock (engine.hpp WsLease)
  std::shared_lock<std::shared_mutex> lk(e.mu);
  lookup_checks(e, cs, proto);
  const int among = candidates ? 1 : 2;
  const size_t n = candidates ? n_candidates : (vary_res ? (size_t)e.interner[proto.resource_type].count : 0);
  const bool hit = lookup_kept(e, proto, vary_res, now_us, among) && g_lookup.cand.size() == (candidates ? n : 0) &&
                   (!candidates || n == 0 || std::memcmp(g_lookup.cand.data(), candidates, n * 4) == 0);
  if (!hit) {
    g_lookup.generation = 0;
    const gck_uniform hdr{proto.resource_type, proto.permission, proto.subject_type, proto.subject_relation, 0, 0};
    CompactReq q{&hdr, 1u, nullptr, nullptr, n, nullptr, nullptr, 0, nullptr};
    q.vary = vary_res ? GCK_VARY_RESOURCE : GCK_VARY_SUBJECT;
    q.fixed_id = vary_res ? proto.subject_id : proto.resource_id;
    q.ids = candidates;
    device_lookup_among(e, p.ws[0], p.ws[1], q, now_us, g_lookup.ids, g_lookup.perms);
    lookup_keep(e, proto, vary_res, now_us, among);
    // (the candidates are remembered only with a result that has to be kept for the retry)
    if (candidates && g_lookup.ids.size() > cap) g_lookup.cand.assign(candidates, candidates + n);
  }
  lookup_copy_out(out_ids, out_perm, cap, out_n);
}

int gck_lookup_resources_among(gck_engine* ge, const gck_consistency* cs, uint16_t resource_type, uint16_t permission,
                               uint16_t subject_type, uint16_t subject_relation, uint32_t subject_id,
                               const uint32_t* candidates, size_t n_candidates, int64_t now_us, uint32_t* out_ids,
                               uint8_t* out_perm, size_t cap, size_t* out_n) {
  return guard([&] {
    REQUIRE(subject_id != GCK_ID_WILDCARD, GCK_E_INVALID_ARGUMENT, "cannot perform lookup on wildcard subject");
    gck_item proto{resource_type, permission, 0, subject_type, subject_relation, subject_id, 0};
    lookup_among(ge, cs, proto, true, candidates, n_candidates, now_us, out_ids, out_perm, cap, out_n);
  });
}

int gck_lookup_subjects_among(gck_engine* ge, const gck_consistency* cs, uint16_t resource_type, uint32_t resource_id,
                              uint16_t permission, uint16_t subject_type, uint16_t subject_relation,
                              const uint32_t* candidates, size_t n_candidates, int64_t now_us, uint32_t* out_ids,
                              uint8_t* out_perm, size_t cap, size_t* out_n) {
  return guard([&] {
    gck_item proto{resource_type, permission, resource_id, subject_type, subject_relation, 0, 0};
    lookup_among(ge, cs, proto, false, candidates, n_candidates, now_us, out_ids, out_perm, cap, out_n);
  });
}

int gck_last_stats(gck_engine* ge, gck_stats* out) {
  return guard([&] {
    Engine& e = need(ge);
    REQUIRE(out, GCK_E_INVALID_ARGUMENT, "null out");
    *out = e.stats;
  });
}

int gck_set_profile(gck_engine* ge, uint32_t on) {
  return guard([&] {
    Engine& e = need(ge);
    std::unique_lock<std::shared_mutex> lk(e.mu);  // no batch is being submitted
    if (on) e.cfg.flags |= GCK_FLAG_PROFILE;
    else e.cfg.flags &= ~GCK_FLAG_PROFILE;
  });
}

int gck_reset_stats(gck_engine* ge) {
  return guard([&] {
    Engine& e = need(ge);
    e.stats = gck_stats{};
  });
}

// Test hooks (gck_test_*: not in gck.h, no part of the ABI): the user-slot packing the slot-build
// kernels run (slot_pack.hpp), on the host. gck_test_slot_window: where the omitted run of m sorted
// unique entries begins when n_in stay inline. gck_test_slot_pack: n raw entries (sorted and
// deduplicated in a copy; more than kSlotSortMax: a plain list of n) into the 16 words of a slot at
// `bits` (24 or 32), as user_slot_listed does for more entries than a slot's cap; returns the number
// of entries the list holds, or -1 for bad arguments.
uint32_t gck_test_slot_window(const uint32_t* e, uint32_t m, uint32_t n_in) { return gck::slot_window(e, m, n_in); }

int gck_test_slot_pack(uint32_t bits, const uint32_t* raw, uint32_t n, uint32_t list_at, uint32_t* w) {
  if ((bits != 24 && bits != 32) || n > gck::kSlotCount || !raw || !w) return -1;
  if (n > gck::kSlotSortMax) {
    gck::slot_pack_plain_list(bits, n, list_at, w);
    return (int)n;
  }
  uint32_t e[gck::kSlotSortMax];
  for (uint32_t k = 0; k < n; ++k) e[k] = raw[k];
  const uint32_t m = gck::slot_sort_unique(e, n);
  gck::slot_pack_sorted(bits, e, m, list_at, w);
  return (int)m;
}

// gck_test_front_pack: the 16-B front (slot_pack.hpp) of the 16-word resource slot `slot`, as the
// slot-build kernel writes it, into front[4]; when it packed, the 8 slot words it stands for into
// unpacked[8] (untouched otherwise). Returns 1 packed, 0 flagged "read the slot", -1 bad arguments.
int gck_test_front_pack(const uint32_t* slot, uint32_t* front, uint32_t* unpacked) {
  if (!slot || !front || !unpacked) return -1;
  if (!gck::front_pack(slot, front)) return 0;
  gck::front_unpack(front, unpacked);
  return 1;
}

// gck_test_select_plane: the ordered selection of k_dc_select (select_plane.hpp) over a chunk's plane
// of n_words words on the host, tile by tile as the kernel's blocks take it: a tile's first rank is
// `base` (the request's count before the chunk) plus a recount of the words before the tile, ranks
// inside the tile run on. Survivors' positions and GCK_PERM_* go to out_pos / out_perm (either may
// be null) while their rank is below cap; *out_n = base + the chunk's survivors. -1 for a bad mask
// or null arguments.
int gck_test_select_plane(const uint64_t* words, uint32_t n_words, uint32_t mask, uint32_t base, uint32_t cap,
                          uint32_t* out_pos, uint8_t* out_perm, uint32_t* out_n) {
  if (mask == 0 || (mask & ~0xEu) || (!words && n_words) || !out_n) return -1;
  const gck::SelectOut o{nullptr, out_pos, out_perm, cap, nullptr, 0u, 0u};
  uint32_t total = base;
  for (uint32_t tile0 = 0; tile0 < n_words; tile0 += gck::kSelBlock) {
    uint32_t rank = base + gck::select_count_strided(words, 0, tile0, 1, mask);
    for (uint32_t t = tile0; t < n_words && t < tile0 + gck::kSelBlock; ++t) {
      const uint64_t m = gck::select_mask(words[t], mask);
      gck::select_write(words[t], m, t, rank, o);
      rank += gck::select_count(m);
    }
    total = rank;
  }
  *out_n = total;
  return 0;
}

// gck_test_select_rows: the row-segmented selection of a cross filter request (select_plane.hpp;
// k_dc_rows_count, k_dc_rows_scan and k_dc_rows_write in device_compact.inc) over a row-padded plane
// of S rows of ceil(R / 32) words on the host, with the same functions, row by row and piece by piece
// of kRowPiece words as the kernels walk them: the counts, their prefix, then each word's survivors
// from the in-row rank the words before it give. Outputs and NULL rules are gck_select_rows' (src_ids:
// the resource list, needed with out_ids). -1 for the selection's argument errors. What this pins is
// the per-word functions and the protocol; the kernels' lane scans inside a wave are covered only by
// the GPU tests.
int gck_test_select_rows(const uint64_t* words, uint32_t S, uint32_t R, uint32_t mask, uint32_t row_limit, size_t cap,
                         const uint32_t* src_ids, uint32_t* out_row_off, uint32_t* out_row_n, uint32_t* out_ids,
                         uint32_t* out_col, uint8_t* out_perm, uint32_t* out_n) {
  gck_select_rows sel{mask, row_limit, out_row_off, out_row_n, out_ids, out_col, out_perm, cap, out_n};
  if (select_rows_fault(&sel)) return -1;
  const uint32_t stride = (R + 31u) / 32u;
  if ((!words && S && stride) || (out_ids && !src_ids && R)) return -1;
  if (S && R && S > 0xFFFFFFFFu / R) return -1;
  const gck::SelectRowsOut o{out_ids, out_col, out_perm, (uint32_t)std::min<size_t>(cap, 0xFFFFFFFFu), src_ids};
  const auto row_word = [&](uint32_t s, uint32_t t, uint64_t& word) {
    word = words[(size_t)s * stride + t];
    return gck::select_row_mask(word, mask, t, R);
  };
  for (uint32_t s = 0; s < S; ++s) {  // k_dc_rows_count
    uint32_t sum = 0;
    for (uint32_t p0 = 0; p0 < stride; p0 += gck::kRowPiece)
      for (uint32_t t = p0; t < stride && t < p0 + gck::kRowPiece; ++t) {
        uint64_t word;
        sum += gck::select_count(row_word(s, t, word));
      }
    out_row_off[s + 1u] = gck::select_row_kept(sum, row_limit);
    if (out_row_n) out_row_n[s] = sum;
  }
  uint32_t run = 0;  // k_dc_rows_scan
  for (uint32_t s = 0; s < S; ++s) out_row_off[s + 1u] = run += out_row_off[s + 1u];
  out_row_off[0] = 0u;
  *out_n = run;
  for (uint32_t s = 0; s < S && o.cap; ++s) {  // k_dc_rows_write
    uint32_t carry = 0;
    for (uint32_t p0 = 0; p0 < stride; p0 += gck::kRowPiece) {
      uint32_t rank = carry;
      for (uint32_t t = p0; t < stride && t < p0 + gck::kRowPiece; ++t) {
        uint64_t word;
        const uint64_t m = row_word(s, t, word);
        gck::select_write_row(word, m, t * 32u, rank, out_row_off[s], row_limit, o);
        rank += gck::select_count(m);
      }
      carry = rank;
      if (row_limit && carry >= row_limit) break;
    }
  }
  return 0;
}

// gck_test_select_cols: the column-segmented selection of a cross filter request by resource
// (select_plane.hpp; k_dc_cols_count, k_dc_rows_scan and k_dc_cols_write in device_compact.inc) over a
// row-padded plane of S rows of ceil(R / 32) words on the host, with the same functions and the same
// walk: blocks of kColGroup columns, the rows in tiles of kColTile, each tile's rows of a column in
// kColChunks chunks counted one by one (select_col_walk, in its batches of words) into a block's
// table, the prefix, then each chunk written from the rank the chunks and the tiles before it carry.
// Only the staging differs: the kernels read a tile's words from LDS, this reads them from the plane.
// Outputs and NULL rules are gck_select_cols' (src_ids: the subject list, needed with out_ids). -1 for
// the selection's argument errors. What this does not pin is the staging and the barriers between a
// block's waves: the GPU tests' ground.
int gck_test_select_cols(const uint64_t* words, uint32_t S, uint32_t R, uint32_t mask, uint32_t col_limit, size_t cap,
                         const uint32_t* src_ids, uint32_t* out_col_off, uint32_t* out_col_n, uint32_t* out_ids,
                         uint32_t* out_row, uint8_t* out_perm, uint32_t* out_n) {
  gck_select_cols sel{mask, col_limit, out_col_off, out_col_n, out_ids, out_row, out_perm, cap, out_n};
  if (select_cols_fault(&sel)) return -1;
  const uint32_t stride = (R + 31u) / 32u;
  if ((!words && S && stride) || (out_ids && !src_ids && S)) return -1;
  if (S && R && S > 0xFFFFFFFFu / R) return -1;
  const gck::SelectColsOut o{out_ids, out_row, out_perm, (uint32_t)std::min<size_t>(cap, 0xFFFFFFFFu), src_ids};
  const uint32_t blocks = (R + gck::kColGroup - 1u) / gck::kColGroup;
  // part[chunk][lane] of a block's tile, as the kernels' LDS table; walk: one thread's chunk of the tile at row t0
  uint32_t part[gck::kColChunks][gck::kColGroup];
  const auto walk = [&](uint32_t blk, uint32_t t0, uint32_t T, uint32_t chunk, uint32_t lane, const gck::SelectColsOut* out,
                        uint32_t rank, uint32_t base, uint32_t kept) -> uint32_t {
    const uint32_t c = blk * gck::kColGroup + lane, per = gck::select_col_chunk_rows(T);
    const uint32_t r0 = std::min(T, chunk * per), n = std::min(per, T - r0);
    if (c >= R) return 0u;  // (the kernels stage a zero word for it)
    return gck::select_col_walk(words + (size_t)(t0 + r0) * stride + (c >> 5), stride, R, mask, c, t0 + r0, n, out, rank,
                                base, kept);
  };
  const auto count_tile = [&](uint32_t blk, uint32_t t0, uint32_t T) {
    for (uint32_t chunk = 0; chunk < gck::kColChunks; ++chunk)
      for (uint32_t lane = 0; lane < gck::kColGroup; ++lane)
        part[chunk][lane] = walk(blk, t0, T, chunk, lane, nullptr, 0u, 0u, 0u);
  };
  for (uint32_t blk = 0; blk < blocks; ++blk) {  // k_dc_cols_count
    uint32_t surv[gck::kColGroup] = {};
    for (uint32_t t0 = 0; t0 < S; t0 += std::min(gck::kColTile, S - t0)) {
      count_tile(blk, t0, std::min(gck::kColTile, S - t0));
      for (uint32_t chunk = 0; chunk < gck::kColChunks; ++chunk)
        for (uint32_t lane = 0; lane < gck::kColGroup; ++lane) surv[lane] += part[chunk][lane];
    }
    for (uint32_t lane = 0; lane < gck::kColGroup; ++lane) {
      const uint32_t c = blk * gck::kColGroup + lane;
      if (c >= R) continue;
      out_col_off[c + 1u] = gck::select_row_kept(surv[lane], col_limit);
      if (out_col_n) out_col_n[c] = surv[lane];
    }
  }
  uint32_t run = 0;  // k_dc_rows_scan
  for (uint32_t r = 0; r < R; ++r) out_col_off[r + 1u] = run += out_col_off[r + 1u];
  out_col_off[0] = 0u;
  *out_n = run;
  for (uint32_t blk = 0; blk < blocks && S && o.cap; ++blk) {  // k_dc_cols_write
    uint32_t carry[gck::kColGroup] = {};
    for (uint32_t t0 = 0; t0 < S; t0 += std::min(gck::kColTile, S - t0)) {
      const uint32_t T = std::min(gck::kColTile, S - t0);
      count_tile(blk, t0, T);
      for (uint32_t chunk = 0; chunk < gck::kColChunks; ++chunk)
        for (uint32_t lane = 0; lane < gck::kColGroup; ++lane) {
          const uint32_t c = blk * gck::kColGroup + lane;
          if (c >= R) continue;
          uint32_t rank = carry[lane];
          for (uint32_t k = 0; k < chunk; ++k) rank += part[k][lane];
          const uint32_t base = out_col_off[c], kept = out_col_off[c + 1u] - base;
          if (rank < kept && base + rank < o.cap) walk(blk, t0, T, chunk, lane, &o, rank, base, kept);
        }
      for (uint32_t chunk = 0; chunk < gck::kColChunks; ++chunk)
        for (uint32_t lane = 0; lane < gck::kColGroup; ++lane) carry[lane] += part[chunk][lane];
    }
  }
  return 0;
}

// gck_test_group_of: the group lookup of k_dc_group_pairs (select_plane.hpp select_group_of) for n_k
// positions, on the host; whatever `off` holds, every result is within [0, S - 1]. -1 for S == 0 or
// null arguments.
int gck_test_group_of(const uint32_t* off, uint32_t S, const uint32_t* k, uint32_t n_k, uint32_t* out) {
  if (!off || S == 0 || (n_k && (!k || !out))) return -1;
  for (uint32_t i = 0; i < n_k; ++i) out[i] = gck::select_group_of(off, S, k[i]);
  return 0;
}

// gck_test_groups_rule: the group filter entry points' rule function (groups_fault) over the same
// arguments, reading no buffer: 0 when they are good, -1 when the entry points refuse them.
int gck_test_groups_rule(const gck_uniform* hdr, uint32_t vary, const uint32_t* d_owners, size_t S,
                         const uint32_t* d_group_off, const uint32_t* d_candidates, size_t n, size_t n_contexts,
                         const gck_select_groups* sel, const uint64_t* d_out_packed, const gck_item_error* d_out_errs,
                         size_t err_cap, const uint32_t* d_out_n_errs) {
  return groups_fault(hdr, vary, d_owners, S, d_group_off, d_candidates, n, n_contexts, sel, d_out_packed, d_out_errs,
                      err_cap, d_out_n_errs).empty() ? 0 : -1;
}

// gck_test_select_groups: the group-segmented selection of a group filter request (select_plane.hpp;
// k_dc_groups_count, k_dc_rows_scan and k_dc_groups_write in device_compact.inc) over a dense plane of
// ceil(n / 32) words on the host, with the same functions, group by group and piece by piece of L
// words as the kernels walk them (lanes == 0: the kernels' own choice, select_group_lanes; else a power
// of two within 1 .. 64): the clamped ranges, the counts, their prefix, then each word's survivors from
// the in-group rank the words before it give. Outputs and NULL rules are gck_select_groups' (src_ids:
// the candidate list, needed with out_ids). -1 for the selection's argument errors. What this pins is
// the per-word functions, the clamps and the protocol; the kernels' lane scans inside a wave are
// covered only by the GPU tests.
int gck_test_select_groups(const uint64_t* words, uint32_t n, const uint32_t* off, uint32_t S, uint32_t mask,
                           uint32_t group_limit, size_t cap, uint32_t lanes, const uint32_t* src_ids, uint32_t* out_row_off,
                           uint32_t* out_row_n, uint32_t* out_ids, uint32_t* out_pos, uint8_t* out_perm, uint32_t* out_n) {
  gck_select_groups sel{mask, group_limit, out_row_off, out_row_n, out_ids, out_pos, out_perm, cap, out_n};
  const gck_uniform hdr{};
  static const uint64_t plane0 = 0;  // (the rule wants a plane pointer; the hook's own is checked below)
  if (!groups_fault(&hdr, GCK_VARY_RESOURCE, off, S, off, off, 0, 0, &sel, &plane0, nullptr, 0, nullptr).empty()) return -1;
  if (n && (!words || !off || S == 0 || (out_ids && !src_ids))) return -1;
  if (lanes && (lanes > 64u || (lanes & (lanes - 1u)))) return -1;
  const uint32_t L = lanes ? lanes : gck::select_group_lanes(n, S);
  const gck::SelectRowsOut o{out_ids, out_pos, out_perm, (uint32_t)std::min<size_t>(cap, 0xFFFFFFFFu), src_ids};
  const auto range = [&](uint32_t s, uint32_t& lo, uint32_t& hi, uint32_t& w0, uint32_t& nw) {
    gck::select_group_range(off, s, n, lo, hi);
    w0 = lo >> 5;
    nw = hi > lo ? ((hi - 1u) >> 5) - w0 + 1u : 0u;
  };
  for (uint32_t s = 0; s < S; ++s) {  // k_dc_groups_count
    uint32_t lo, hi, w0, nw, sum = 0;
    range(s, lo, hi, w0, nw);
    for (uint32_t p0 = 0; p0 < nw; p0 += L)
      for (uint32_t t = p0; t < nw && t < p0 + L; ++t)
        sum += gck::select_count(gck::select_group_mask(words[w0 + t], mask, w0 + t, lo, hi));
    out_row_off[s + 1u] = gck::select_row_kept(sum, group_limit);
    if (out_row_n) out_row_n[s] = sum;
  }
  uint32_t run = 0;  // k_dc_rows_scan
  for (uint32_t s = 0; s < S; ++s) out_row_off[s + 1u] = run += out_row_off[s + 1u];
  out_row_off[0] = 0u;
  *out_n = run;
  for (uint32_t s = 0; s < S && n && o.cap; ++s) {  // k_dc_groups_write
    uint32_t lo, hi, w0, nw, carry = 0;
    range(s, lo, hi, w0, nw);
    for (uint32_t p0 = 0; p0 < nw && !(group_limit && carry >= group_limit); p0 += L) {
      uint32_t rank = carry;
      for (uint32_t t = p0; t < nw && t < p0 + L; ++t) {
        const uint64_t word = words[w0 + t], m = gck::select_group_mask(word, mask, w0 + t, lo, hi);
        gck::select_write_row(word, m, (w0 + t) * 32u, rank, out_row_off[s], group_limit, o);
        rank += gck::select_count(m);
      }
      carry = rank;
    }
  }
  return 0;
}

// gck_test_changes_rule / gck_test_row_changes_rule: the recheck entry points' rule functions
// (changes_fault, row_changes_fault) over the same arguments, reading no buffer: 0 when they are
// good, -1 when the entry points refuse them. need_plane: d_out is required (a request call; a
// plane-only call with checks).
int gck_test_changes_rule(const gck_select_changes* sel, const uint64_t* d_prev, const uint64_t* d_out, size_t n,
                          int need_plane) {
  return changes_fault(sel, d_prev, d_out, n, need_plane != 0).empty() ? 0 : -1;
}

int gck_test_row_changes_rule(const gck_select_row_changes* sel, const uint64_t* d_prev, const uint64_t* d_out, size_t S,
                              size_t R, int need_plane) {
  return row_changes_fault(sel, d_prev, d_out, S, R, need_plane != 0).empty() ? 0 : -1;
}

// gck_test_change_plane: the dense diff of a recheck request (select_plane.hpp; k_dc_diff and
// dc_diff_plane in device_compact.inc) over two planes of ceil(n / 32) words on the host, chunk by chunk
// of chunk_words words and tile by tile as the kernel's blocks take a chunk: a tile's first rank is
// the count before the chunk plus a recount of the chunk's words before the tile, ranks inside the tile
// run on, and the count is carried from chunk to chunk. old_words may be null (all zeros). Outputs and
// NULL rules are gck_select_changes' (src_ids: the varying ids, or null for first_id + i). -1 for the
// rule's argument errors. What this pins is the per-word functions, the tail mask and the protocol;
// the kernel's lane scan is covered only by the GPU tests.
int gck_test_change_plane(const uint64_t* old_words, const uint64_t* new_words, uint32_t n, uint32_t transitions,
                          uint32_t chunk_words, size_t cap, const uint32_t* src_ids, uint32_t first_id, uint32_t* out_ids,
                          uint32_t* out_pos, uint8_t* out_trans, uint32_t* out_n) {
  gck_select_changes sel{transitions, 0u, out_ids, out_pos, out_trans, cap, out_n};
  if (!changes_fault(&sel, old_words, new_words, n, n != 0).empty() || chunk_words == 0) return -1;
  const uint32_t words = n / 32u + (n % 32u != 0);
  uint32_t total = 0;
  for (uint32_t w0 = 0; w0 < words; w0 += std::min(chunk_words, words - w0)) {  // dc_diff_plane's chunks
    const uint32_t cw = std::min(chunk_words, words - w0), pos = w0 * 32u, cn = std::min(cw * 32u, n - pos);
    const uint64_t* o_ = old_words ? old_words + w0 : nullptr;
    const uint64_t* n_ = new_words + w0;
    const gck::ChangeOut o{out_ids, out_pos, out_trans, (uint32_t)std::min<size_t>(cap, 0xFFFFFFFFu),
                           src_ids ? src_ids + pos : nullptr, src_ids ? 0u : first_id + pos, pos};
    const uint32_t base = total;
    for (uint32_t tile0 = 0; tile0 < cw; tile0 += gck::kSelBlock) {  // k_dc_diff's blocks
      uint32_t rank = base + gck::change_count_strided(o_, n_, 0, tile0, 1, transitions, cn);
      for (uint32_t t = tile0; t < cw && t < tile0 + gck::kSelBlock; ++t) {
        const uint64_t ow = o_ ? o_[t] : 0ull, m = gck::change_tail_mask(ow, n_[t], transitions, t, cn);
        gck::change_write(ow, n_[t], m, t, rank, o);
        rank += gck::select_count(m);
      }
      total = rank;
    }
  }
  *out_n = total;
  return 0;
}

// gck_test_change_rows: the row form (k_dc_diff_rows_count, k_dc_rows_scan and k_dc_diff_rows_write)
// over two row-padded planes of S rows of ceil(R / 32) words on the host, row by row and piece by
// piece of kRowPiece words as the kernels walk them: the counts, their prefix, then each word's changes
// from the in-row rank the words before it give. Outputs and NULL rules are gck_select_row_changes'
// (src_ids: the resource list, needed with out_ids). -1 for the rule's argument errors.
int gck_test_change_rows(const uint64_t* old_words, const uint64_t* new_words, uint32_t S, uint32_t R, uint32_t transitions,
                         size_t cap, const uint32_t* src_ids, uint32_t* out_row_off, uint32_t* out_ids, uint32_t* out_col,
                         uint8_t* out_trans, uint32_t* out_n) {
  gck_select_row_changes sel{transitions, 0u, out_row_off, out_ids, out_col, out_trans, cap, out_n};
  if (!row_changes_fault(&sel, old_words, new_words, S, R, S != 0 && R != 0).empty()) return -1;
  if (out_ids && !src_ids && R) return -1;
  if (S && R && S > 0xFFFFFFFFu / R) return -1;
  const uint32_t stride = R / 32u + (R % 32u != 0);
  const gck::ChangeRowsOut o{out_ids, out_col, out_trans, (uint32_t)std::min<size_t>(cap, 0xFFFFFFFFu), src_ids};
  const auto row_word = [&](uint32_t s, uint32_t t, uint64_t& ow, uint64_t& nw) {
    const size_t at = (size_t)s * stride + t;
    nw = new_words[at];
    ow = old_words ? old_words[at] : 0ull;
    return gck::change_row_mask(ow, nw, transitions, t, R);
  };
  for (uint32_t s = 0; s < S; ++s) {  // k_dc_diff_rows_count
    uint32_t sum = 0;
    for (uint32_t p0 = 0; p0 < stride; p0 += gck::kRowPiece)
      for (uint32_t t = p0; t < stride && t < p0 + gck::kRowPiece; ++t) {
        uint64_t ow, nw;
        sum += gck::select_count(row_word(s, t, ow, nw));
      }
    out_row_off[s + 1u] = sum;
  }
  uint32_t run = 0;  // k_dc_rows_scan
  for (uint32_t s = 0; s < S; ++s) out_row_off[s + 1u] = run += out_row_off[s + 1u];
  out_row_off[0] = 0u;
  *out_n = run;
  for (uint32_t s = 0; s < S && stride && o.cap; ++s) {  // k_dc_diff_rows_write
    uint32_t carry = 0;
    for (uint32_t p0 = 0; p0 < stride; p0 += gck::kRowPiece) {
      uint32_t rank = carry;
      for (uint32_t t = p0; t < stride && t < p0 + gck::kRowPiece; ++t) {
        uint64_t ow, nw;
        const uint64_t m = row_word(s, t, ow, nw);
        gck::change_write_row(ow, nw, m, t * 32u, rank, out_row_off[s], o);
        rank += gck::select_count(m);
      }
      carry = rank;
    }
  }
  return 0;
}

}  // extern "C"
