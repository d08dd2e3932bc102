// labels_build.inc — the host side of the label join (labels.inc): the build of its tables for a
// snapshot. Hubs and the hierarchy's labels, the Watch dirty path, then build_labels: a list of
// stages over one LjBuild (plan, keys and adoption, host rows, hierarchy, arrow forest, sizing, user
// slots, resource slots, commit). Host code only: the kernels it launches are in labels.inc,
// closure.inc and bidir.inc. Included by engine.hip after labels.inc.

// Tree labels and covers of a DAG given as parents per vertex (the same construction as
// bidir.inc build_ancestors, over any vertex set): lab[2v] = pre(v) | overflow << 31,
// lab[2v + 1] = end(v), cov_off / cov_pre the covers' preorder numbers. False on a cycle.
static bool hier_labels(uint32_t n, const std::vector<uint32_t>& poff, const std::vector<uint32_t>& pnbr,
                        const std::vector<uint32_t>& coff_all, const std::vector<uint32_t>& cnbr_all,
                        std::vector<uint32_t>& lab, std::vector<uint32_t>& cov_off, std::vector<uint32_t>& cov_pre) {
  TopoLevels T;
  if (!topo_levels(n, poff, coff_all.data(), cnbr_all.data(), T)) return false;
  tree_labels(n, poff, pnbr, T, kLjCoverMax, host_threads(), lab, cov_off, cov_pre);
  return true;
}

// Strongly connected components of the hierarchy (iterative Tarjan over the child lists):
// comp[v] in [0, n_comp). Vertices of one component reach each other, so they share their upward
// closure; the labels are built over the condensed DAG. (Checks whose resource reaches a cycle sit
// at the depth budget and are deferred by the height guard; everything else stays exact.)
// `trivial`: vertices known to lie on no cycle (Kahn's order reached them: their parents all
// came first), each its own component without a visit — a remaining vertex's children are
// remaining too (an edge into a Kahn-ordered vertex would have held it back), so Tarjan runs over
// the remaining ones alone: the cycles and what lies below them.
static uint32_t hier_scc(uint32_t n, const std::vector<uint32_t>& coff, const std::vector<uint32_t>& cnbr,
                         const std::vector<char>& trivial, std::vector<uint32_t>& comp) {
  constexpr uint32_t kUnset = 0xFFFFFFFFu;
  std::vector<uint32_t> index(n, kUnset), low(n, 0), stack, it_pos(n, 0), call;
  std::vector<char> on(n, 0);
  comp.assign(n, kUnset);
  uint32_t next_index = 0, n_comp = 0;
  for (uint32_t s = 0; s < n; ++s)
    if (trivial[s]) index[s] = next_index++, comp[s] = n_comp++;
  for (uint32_t s = 0; s < n; ++s) {
    if (index[s] != kUnset) continue;
    call.push_back(s);
    index[s] = low[s] = next_index++;
    stack.push_back(s);
    on[s] = 1;
    it_pos[s] = coff[s];
    while (!call.empty()) {
      const uint32_t v = call.back();
      if (it_pos[v] < coff[v + 1]) {
        const uint32_t w = cnbr[it_pos[v]++];
        if (index[w] == kUnset) {
          index[w] = low[w] = next_index++;
          stack.push_back(w);
          on[w] = 1;
          it_pos[w] = coff[w];
          call.push_back(w);
        } else if (on[w]) {
          low[v] = std::min(low[v], index[w]);
        }
        continue;
      }
      call.pop_back();
      if (!call.empty()) low[call.back()] = std::min(low[call.back()], low[v]);
      if (low[v] == index[v]) {
        for (;;) {
          const uint32_t w = stack.back();
          stack.pop_back();
          on[w] = 0;
          comp[w] = n_comp;
          if (w == v) break;
        }
        ++n_comp;
      }
    }
  }
  return n_comp;
}

// Tree labels and covers of any hierarchy (cycles condensed): per vertex lab[2v] / lab[2v + 1]
// and its cover (cov_off / cov_pre), those of its component.
static void hier_labels_any(uint32_t n, const std::vector<uint32_t>& poff, const std::vector<uint32_t>& pnbr,
                            const std::vector<uint32_t>& coff, const std::vector<uint32_t>& cnbr, std::vector<uint32_t>& lab,
                            std::vector<uint32_t>& cov_off, std::vector<uint32_t>& cov_pre, uint32_t& n_cyclic) {
  n_cyclic = 0;
  PhaseClock pc("hier");
  if (hier_labels(n, poff, pnbr, coff, cnbr, lab, cov_off, cov_pre)) return;
  pc.mark("acyclic_try");
  std::vector<char> trivial(n, 0);
  {  // Kahn's order over the whole hierarchy: what it reaches lies on no cycle
    std::vector<uint32_t> indeg(n), q;
    q.reserve(n);
    for (uint32_t v = 0; v < n; ++v)
      if (!(indeg[v] = poff[v + 1] - poff[v])) q.push_back(v);
    for (size_t qi = 0; qi < q.size(); ++qi) {
      trivial[q[qi]] = 1;
      for (uint32_t k = coff[q[qi]]; k < coff[q[qi] + 1]; ++k)
        if (--indeg[cnbr[k]] == 0) q.push_back(cnbr[k]);
    }
  }
  std::vector<uint32_t> comp;
  const uint32_t nc = hier_scc(n, coff, cnbr, trivial, comp);
  pc.mark("scc");
  std::vector<uint32_t> csize(nc, 0);
  for (uint32_t v = 0; v < n; ++v) ++csize[comp[v]];
  for (uint32_t v = 0; v < n; ++v) n_cyclic += csize[comp[v]] > 1 ? 1u : 0u;
  // the condensed DAG (parent comp -> child comp, deduplicated): the edges bucketed by parent
  // component (a counting sort), each bucket sorted and deduplicated in parallel, then the
  // parents lists from the children lists
  std::vector<uint32_t> bo((size_t)nc + 1, 0), bk;
  for (uint32_t v = 0; v < n; ++v)
    for (uint32_t k = coff[v]; k < coff[v + 1]; ++k)
      if (comp[v] != comp[cnbr[k]]) ++bo[comp[v] + 1];
  for (uint32_t c = 0; c < nc; ++c) bo[c + 1] += bo[c];
  bk.resize(bo[nc]);
  {
    std::vector<uint32_t> at(bo.begin(), bo.end() - 1);
    for (uint32_t v = 0; v < n; ++v)
      for (uint32_t k = coff[v]; k < coff[v + 1]; ++k)
        if (comp[v] != comp[cnbr[k]]) bk[at[comp[v]]++] = comp[cnbr[k]];
  }
  std::vector<uint32_t> blen(nc, 0);
  parallel_chunks(nc, host_threads(), [&](unsigned, size_t lo, size_t hi) {
    for (size_t c = lo; c < hi; ++c) {
      std::sort(bk.begin() + bo[c], bk.begin() + bo[c + 1]);
      blen[c] = (uint32_t)(std::unique(bk.begin() + bo[c], bk.begin() + bo[c + 1]) - (bk.begin() + bo[c]));
    }
  });
  std::vector<uint32_t> qcoff((size_t)nc + 1, 0);
  for (uint32_t c = 0; c < nc; ++c) qcoff[c + 1] = qcoff[c] + blen[c];
  std::vector<uint32_t> qcnbr(qcoff[nc]), qpoff((size_t)nc + 1, 0), qpnbr(qcoff[nc]);
  for (uint32_t c = 0; c < nc; ++c) {
    std::copy(bk.begin() + bo[c], bk.begin() + bo[c] + blen[c], qcnbr.begin() + qcoff[c]);
    for (uint32_t k = 0; k < blen[c]; ++k) ++qpoff[bk[bo[c] + k] + 1];
  }
  for (uint32_t c = 0; c < nc; ++c) qpoff[c + 1] += qpoff[c];
  {
    std::vector<uint32_t> pa(qpoff.begin(), qpoff.end() - 1);
    for (uint32_t c = 0; c < nc; ++c)  // (parents in ascending order, as the sorted edge list gave them)
      for (uint32_t k = qcoff[c]; k < qcoff[c + 1]; ++k) qpnbr[pa[qcnbr[k]]++] = c;
  }
  pc.mark("condense");
  std::vector<uint32_t> clab, ccoff, ccpre;
  if (!hier_labels(nc, qpoff, qpnbr, qcoff, qcnbr, clab, ccoff, ccpre))
    throw Error(GCK_E_DEVICE, "engine invariant violated: condensed hierarchy is cyclic");
  lab.assign(2 * (size_t)n, 0);
  cov_off.assign((size_t)n + 1, 0);
  const unsigned nt = host_threads();
  parallel_chunks(n, nt, [&](unsigned, size_t lo, size_t hi) {
    for (size_t v = lo; v < hi; ++v) {
      const uint32_t c = comp[v];
      lab[2 * v] = clab[2 * (size_t)c];
      lab[2 * v + 1] = clab[2 * (size_t)c + 1];
      cov_off[v + 1] = ccoff[c + 1] - ccoff[c];
    }
  });
  for (uint32_t v = 0; v < n; ++v) cov_off[v + 1] += cov_off[v];
  cov_pre.resize(cov_off[n]);
  parallel_chunks(n, nt, [&](unsigned, size_t lo, size_t hi) {
    for (size_t v = lo; v < hi; ++v)
      std::copy(ccpre.begin() + ccoff[comp[v]], ccpre.begin() + ccoff[comp[v] + 1], cov_pre.begin() + cov_off[v]);
  });
  pc.mark("labels_expand");
}

namespace {

struct HostRows {  // a host copy of one CSR of the snapshot
  std::vector<uint32_t> off, nbr;
  std::vector<uint32_t> cav;  // ext CSRs: caveat instance and expiry per edge
  std::vector<int64_t> exp;
  uint32_t n_rows = 0;
};

// One flattened term of one resource: users reached without entering a hub, hub vertices entered,
// a wildcard.
struct Flat {
  std::vector<uint32_t> D, V;
  std::vector<uint32_t> C;  // (user | kLjCav, instance) pairs: reached only through a partial caveat
  bool wild = false, over = false;
};

// One step of a term's walk over the node program (walk_term): a node entered (item == kNone),
// or one of its items; `far`: on another object than the resource's own (through an arrow or a
// userset).
struct TermVisit {
  uint32_t node, item;
  bool far;
};

struct LabelPlan {
  uint32_t p;                    // the root (a permission node, or a hub: no terms)
  std::vector<uint32_t> terms;   // operand nodes
  std::vector<TermVisit> walk;   // the walks of its terms, one after another
  uint8_t neg = 0;
  bool cav = false;              // a term reads caveated relationships (the caveat plane)
  uint32_t sw_need = 16;         // slot words the sample asked for
};

}  // namespace

// Hubs of a node program (over its forward nodes [0, nf)): targets of usersets and arrows that are
// unions of stored subjects and computed usersets, whose usersets point at hubs again, with no
// caveated / expiring edge (`ext(item index)`). loc[h]: the nodes of hub h on its own object.
template <class Ext>
static void find_hubs(const std::vector<DevNode>& nodes, const std::vector<DevItem>& items, uint32_t nf, Ext&& ext,
                      std::vector<char>& hub, std::vector<std::vector<uint32_t>>& loc) {
  std::vector<char> target(nf, 0);
  hub.assign(nf, 0);
  loc.assign(nf, {});
  for (uint32_t n = 0; n < nf; ++n)
    for (uint32_t k = 0; k < nodes[n].count; ++k) {
      const DevItem& it = items[nodes[n].first + k];
      if ((it.kind == IT_KIND && it.srel != kEllipsis) || it.kind == IT_ARROW)
        if (it.target != kNoNode && it.target < nf) target[it.target] = 1;
    }
  for (uint32_t h = 0; h < nf; ++h) {
    if (!target[h]) continue;
    std::vector<uint32_t> stack{h}, out;
    std::vector<char> seen(nf, 0);
    seen[h] = 1;
    bool ok = true;
    while (!stack.empty() && ok) {
      const uint32_t n = stack.back();
      stack.pop_back();
      out.push_back(n);
      const DevNode& nd = nodes[n];
      if (nd.kind != NK_RELATION && nd.kind != NK_UNION && nd.kind != NK_NIL) ok = false;
      for (uint32_t k = 0; k < nd.count && ok; ++k) {
        const DevItem& it = items[nd.first + k];
        if (nd.kind == NK_UNION) {
          if (it.kind != IT_COMPUTED || it.target >= nf) ok = false;
          else if (!seen[it.target]) seen[it.target] = 1, stack.push_back(it.target);
        } else if (it.kind != IT_KIND || ext(nd.first + k)) {
          ok = false;
        }
      }
    }
    if (ok) {
      hub[h] = 1;
      loc[h] = std::move(out);
    }
  }
  for (bool changed = true; changed;) {  // a hub's usersets must point at hubs
    changed = false;
    for (uint32_t h = 0; h < nf; ++h) {
      if (!hub[h]) continue;
      for (uint32_t n : loc[h])
        for (uint32_t k = 0; k < nodes[n].count && hub[h]; ++k) {
          const DevItem& it = items[nodes[n].first + k];
          if (nodes[n].kind == NK_RELATION && it.srel != kEllipsis && (it.target >= nf || !hub[it.target])) {
            hub[h] = 0;
            changed = true;
          }
        }
    }
  }
}

// The ingest rules of a partitioned graph (SURVEY §8e; engine.hpp part_keep), from the schema
// alone, so that every rank filters the export stream (client/client.go:472-499) and the Watch
// stream the same way: the hubs a label join can meet are those of the schema whose relations
// allow no caveat or expiration; the relations of those hubs are the hierarchy — their userset
// (and wildcard) tuples are replicated on every rank, their direct-subject tuples are kept also by
// the subject's owner (the subject side of the join, the user slots).
void partition_rules(Engine& e) {
  e.part_hub_node.clear();
  e.part_hub_rel.clear();
  e.part_sub_node.clear();
  if (!e.schema) return;
  const Schema& sc = *e.schema;
  const uint32_t nf = (uint32_t)sc.nodes.size();
  auto ext = [&](uint32_t i) {
    const DevItem& it = sc.items[i];
    const uint16_t rel = sc.item_rel[i];
    if (rel >= sc.rels.size()) return true;
    for (const Allowed& a : sc.rels[rel].allowed)
      if (a.stype == it.stype && a.srel == it.srel && (!a.caveat.empty() || a.expiration)) return true;
    return false;
  };
  std::vector<char> hub;
  std::vector<std::vector<uint32_t>> loc;
  find_hubs(sc.nodes, sc.items, nf, ext, hub, loc);
  // A hub relation's direct tuples live with their subjects' owners, which is right only if every
  // node that reads its rows is one of the hubs' nodes (routed there, partition.inc part_dest). A
  // hub whose relation is also read elsewhere — e.g. as an arrow's tupleset by a permission outside
  // the hub — is no hub of the partition (its rows stay with their objects' owners, its roots go to
  // the level loop); dropping one changes which nodes are hub nodes, so repeat until none is read
  // from outside.
  for (bool changed = true; changed;) {
    changed = false;
    e.part_hub_rel.assign(sc.rels.size(), 0);
    e.part_sub_node.assign(nf, 0);
    for (uint32_t h = 0; h < nf; ++h)
      if (hub[h])
        for (uint32_t n : loc[h]) {
          e.part_sub_node[n] = 1;
          if (n < sc.rels.size() && sc.nodes[n].kind == NK_RELATION) e.part_hub_rel[n] = 1;
        }
    std::vector<char> bad(sc.rels.size(), 0);
    for (uint32_t n = 0; n < nf; ++n) {
      if (e.part_sub_node[n]) continue;
      for (uint32_t k = 0; k < sc.nodes[n].count; ++k) {
        const uint32_t i = sc.nodes[n].first + k;
        const uint8_t kind = sc.items[i].kind;
        if (kind != IT_KIND && kind != IT_ARROW) continue;
        const uint16_t rel = sc.item_rel[i];
        if (rel < bad.size() && e.part_hub_rel[rel]) bad[rel] = 1;
      }
    }
    for (uint32_t h = 0; h < nf; ++h) {
      if (!hub[h]) continue;
      for (uint32_t n : loc[h])
        if (n < bad.size() && bad[n]) {
          hub[h] = 0;
          changed = true;
          break;
        }
    }
  }
  e.part_hub_node.assign(hub.begin(), hub.end());
}

// May a Watch batch keep the current label tables although some of their CSRs changed? When every
// changed one is a direct-grant CSR (`dkey`, the users listed in resource slots) that the batch
// merged (Engine::delta_hint), no wildcard grant changed, no root's resource crossed the depth
// budget: the checks of the subjects whose grants
// changed then go to the wave bundles (k_label_join reads the dirty set), everything else the
// tables answer as before — a 0.1 % churn of direct grants (BASELINE config 5) rebuilds nothing.
// Not on a partitioned graph (its slots live on several ranks).
// `own_only`: the direct-grant CSRs every root reads only on its resource's own object (a changed
// wildcard grant there changes that resource alone). `why`: the reason a rebuild is needed.
static bool lj_dirty_path(const Engine& e, const DeviceSnapshot& ds, const std::vector<uint64_t>& dkey,
                          const std::vector<const uint32_t*>& hkey, uint32_t max_depth,
                          const std::vector<uint32_t>& own_only, const std::vector<uint32_t>& hroots,
                          const char*& why) {
  const DeviceSnapshot& old = *e.dev;
  why = "not a Watch batch";
  if (!e.delta_hint || e.part_world > 1) return false;
  why = "other grant CSRs";
  if (old.lj.dkey.size() != dkey.size() || old.lj.hgt.size() != hkey.size()) return false;
  uint64_t marks = 0;
  for (size_t q = 0; q < dkey.size(); q += 4) {
    if (old.lj.dkey[q] != dkey[q]) return false;  // (another CSR)
    if (old.lj.dkey[q + 1] == dkey[q + 1] && old.lj.dkey[q + 2] == dkey[q + 2]) continue;
    const DeltaHint::Fwd* f = nullptr;
    for (const DeltaHint::Fwd& x : e.delta_hint->fwd)
      if ((uint64_t)(uintptr_t)x.nbr == dkey[q + 1]) f = &x;
    why = "a grant CSR the batch did not merge";
    if (!f) return false;
    why = "a wildcard grant read beyond its own object";
    if (f->wild && !std::binary_search(own_only.begin(), own_only.end(), (uint32_t)dkey[q])) return false;
    marks += f->D;
  }
  // (No rebuild for dirtiness: a dirty subject's checks cost the bundles' time, as without the
  // tables, while a rebuild — 0.45 s for config 2's 2.2M resources — would not pay for itself in
  // ten thousand batches.)
  (void)marks;
  // heights: a changed array must leave every resource on the same side of the budget
  for (size_t k = 0; k < hkey.size(); ++k) {
    if (old.lj.hgt[k] == hkey[k]) continue;
    if (!old.lj.hgt[k] || !hkey[k]) return false;
    const uint32_t p = hroots[k];  // (no resource of the root near the budget before or after)
    if (p < old.hmax.size() && p < ds.hmax.size() && old.hmax[p] < max_depth && ds.hmax[p] < max_depth) continue;
    uint32_t n = 0;
    for (uint32_t p = 0; p < ds.hgt.size(); ++p)
      if (ds.hgt[p] == hkey[k]) n = ds.hcount[p];
    uint32_t n_old = 0;
    for (uint32_t p = 0; p < old.hgt.size(); ++p)
      if (old.hgt[p] == old.lj.hgt[k]) n_old = old.hcount[p];
    why = "heights";
    if (n != n_old) return false;
    std::vector<void*> tmp;
    unsigned hv = 0;
    try {
      unsigned* flag = dalloc<unsigned>(tmp, 1);
      HIP_OK(hipMemset(flag, 0, 4));
      if (n) hipLaunchKernelGGL(k_deep_diff, dim3(grid_for(n)), dim3(kBlock), 0, 0, old.lj.hgt[k], hkey[k], n, max_depth, flag);
      HIP_OK(hipGetLastError());
      HIP_OK(hipMemcpy(&hv, flag, 4, hipMemcpyDeviceToHost));
    } catch (...) {
      free_list(tmp);
      throw;
    }
    free_list(tmp);
    if (hv) return false;
  }
  return true;
}

// An array of the label tables: allocated with the snapshot (bidir.inc slot_alloc, which counts it
// in ds.bytes), recorded in the tables that own it and counted in their size.
static uint32_t* lj_alloc(DeviceSnapshot& ds, LjTables& t, size_t bytes) {
  uint32_t* q = slot_alloc(ds, bytes);
  t.ptrs.push_back(q);
  t.bytes += bytes;
  return q;
}

// Frees the arrays of tables that were never committed, and takes them out of the snapshot's books.
static void lj_release(DeviceSnapshot& ds, LjTables& t) {
  for (void* q : t.ptrs) {
    auto h = std::find(ds.hallocs.begin(), ds.hallocs.end(), q);
    auto a = std::find(ds.allocs.begin(), ds.allocs.end(), q);
    if (h != ds.hallocs.end()) ds.hallocs.erase(h), (void)hipFree(q);
    else if (a != ds.allocs.end()) ds.allocs.erase(a), (void)hipFreeAsync(q, nullptr);
  }
  ds.bytes -= t.bytes;
  t = LjTables{};
}

// Marks the subjects whose direct grants the batch changed (lj_dirty_path held): the dirty set is
// shared with the current snapshot — bits are only ever set, and a check of the current revision
// that sees one goes to the bundles, which answer it from that revision's CSRs.
static void lj_mark_dirty(Engine& e, DeviceSnapshot& ds, const std::vector<uint64_t>& dkey,
                          const std::map<uint32_t, std::vector<uint32_t>>& own_roots) {
  const DeviceSnapshot& old = *e.dev;
  const uint32_t n_users = ds.lj.users;
  auto zeroed = [&](size_t bytes) {
    uint32_t* q = lj_alloc(ds, ds.lj, bytes);
    HIP_OK(hipMemset(q, 0, bytes));
    return q;
  };
  if (!ds.lj.dirty) ds.lj.dirty = zeroed(((size_t)n_users / 32 + 1) * 4);
  // the changed objects of each dirty subject (kDovWords per subject)
  if (ds.lj.af && !ds.lj.dov) ds.lj.dov = zeroed(((size_t)n_users + 1) * kDovWords * 4);
  LjMarks m{};
  m.n_users = n_users;
  m.bits = ds.lj.dirty;
  m.dov = ds.lj.dov;
  auto flush = [&]() {
    if (!m.n) return;
    hipLaunchKernelGGL(k_lj_marks, dim3(m.start[m.n]), dim3(kBlock), 0, 0, m);
    m.n = 0;
  };
  auto add = [&](const DeltaHint::Fwd& f, uint32_t* rslot, uint32_t r_rows, const uint32_t* xlab, uint32_t x_rows,
                 uint32_t wmode) {
    if (m.n == (uint32_t)kLjMarkJobs) flush();
    LjMarkJob& J = m.j[m.n];
    J = LjMarkJob{f.keys, f.ins, f.found, rslot, xlab, f.D, r_rows, ds.lj.sw, x_rows, wmode};
    m.start[m.n + 1] = m.start[m.n] + grid_for(f.D);
    ++m.n;
  };
  // the forest labels of a direct-grant CSR's rows (its relation's resource type)
  auto xlab_of = [&](uint32_t c, uint32_t& rows) -> const uint32_t* {
    rows = 0;
    if (!ds.lj.af) return nullptr;
    for (auto& [cc, t] : ds.lj.dtype)
      if (cc == c && t < ds.lj.af_base.size() && ds.lj.af_base[t] != kNone) {
        rows = ds.lj.af_rows[t];
        return ds.lj.af + 2 * (size_t)ds.lj.af_base[t];
      }
    return nullptr;
  };
  for (size_t q = 0; q < dkey.size(); q += 4) {
    if (old.lj.dkey[q + 1] == dkey[q + 1] && old.lj.dkey[q + 2] == dkey[q + 2]) continue;
    uint32_t x_rows = 0;
    const uint32_t* xlab = xlab_of((uint32_t)dkey[q], x_rows);
    for (const DeltaHint::Fwd& f : e.delta_hint->fwd)
      if ((uint64_t)(uintptr_t)f.nbr == dkey[q + 1] && f.D) {
        add(f, nullptr, 0u, xlab, x_rows, 0u);
        ds.lj.dirty_n += f.D;
        auto ro = own_roots.find((uint32_t)dkey[q]);
        if (f.wild && ro != own_roots.end())  // (lj_dirty_path: read on the resource's own object only)
          for (uint32_t p : ro->second) {
            const uint16_t d = reinterpret_cast<const uint16_t*>(ds.lj.host.data())[p];
            if (d == 0xFFFFu) continue;
            LjMeta M;
            std::memcpy(&M, ds.lj.host.data() + ds.lj.o_meta + (size_t)d * sizeof(LjMeta), sizeof(LjMeta));
            // (a chain program: the walk reads the wildcard's current grants, lj_redecide)
            const uint32_t wmode = !M.chain || !ds.lj.afp ? 0u : M.n_terms < 3u ? 1u : 2u;
            if (M.n_terms) add(f, const_cast<uint32_t*>(M.rslot), M.r_rows, nullptr, 0u, wmode);
          }
      }
  }
  flush();
  // (no synchronisation: the marks are ordered on the null stream before the publication, and
  // the delta arena they read is rewritten only by the next batch, behind them on that stream)
  HIP_OK(hipGetLastError());
}

// ---- build_labels: the stages ---------------------------------------------------------------------

// What the stages of build_labels share. Arrays allocated on the way are recorded in `out`, which
// the commit stage moves into ds.lj; whatever `out` still holds when the build ends — a refusal, an
// exception — is freed.
struct LjBuild {
  Engine& e;
  DeviceSnapshot& ds;
  const std::vector<DevNode>& nodes;
  const std::vector<DevItem>& items;
  const std::vector<DevCSR>& table;
  const std::vector<CsrInfo>& info;
  // a partitioned graph (world > 1) holds this rank's rows and the replicated hub hierarchy: it
  // builds the slots of the subjects and resources it owns, indexed by part_local (the resource
  // side flattens within its own rows and the hubs, and defers a resource whose walk leaves them)
  const uint32_t P, prank, nf, max_depth;
  PhaseClock pc{"labels"};
  uint32_t U = 0;                          // the subject type
  std::vector<char> hub, used;             // hubs of the node program; those the roots reach
  std::vector<std::vector<uint32_t>> loc;  // the hub's nodes on its own object (computed usersets)
  std::vector<LabelPlan> plans;
  std::vector<uint32_t> csrs_all;          // every CSR the flattening and the hierarchy read
  std::vector<uint32_t> dfeed;             // CSRs of direct subjects: they feed only the resource slots' user lists
  std::vector<std::pair<uint32_t, uint16_t>> dfeed_type;  // ... and the type of their rows
  // which roots read each direct-grant CSR on their resource's own object (through computed
  // usersets only), and which CSRs some root reads further away (through an arrow or a userset)
  std::map<uint32_t, std::vector<uint32_t>> own_roots;
  std::set<uint32_t> remote;
  std::vector<uint64_t> key, dkey;         // LjTables::key / dkey / hgt of this build
  std::vector<const uint32_t*> hkey;
  std::unordered_map<uint32_t, HostRows> rows;
  // the hierarchy: one vertex per object of every hub used, x -> y when x lists y#h'
  std::vector<uint64_t> base;
  uint32_t NV = 0, bits = 24;
  std::vector<uint32_t> lab, cov_off, cov_pre;
  std::vector<std::pair<uint32_t, uint64_t>> dsrc;  // (direct-subject CSR of a hub, its vertex base)
  bool any_hub_root = false;
  // the arrow forest (lj_stage_forest); empty: none
  std::vector<uint32_t> af_base, af_rows, af_lab;
  std::vector<uint32_t> par, via;  // per forest vertex: its parent (kNone: a root), the CSR of that edge
  bool pack = false;               // inline slots of 24-bit fields (LjEnt24)
  uint32_t sw = 16;                // slot words
  std::vector<std::vector<uint32_t>> hgt_host;  // per root its resources' heights
  const uint32_t* uslot = nullptr;
  const uint32_t* ulist = nullptr;
  const uint32_t* lab_dev = nullptr;
  std::vector<LjMeta> metas;
  std::vector<uint16_t> root;      // per forward node its LjMeta (0xFFFF: none)
  uint64_t hash = 0xcbf29ce484222325ull;  // GCK_DEBUG_PHASES: FNV-1a of the host-side arrays, in upload order
  LjTables out;

  ~LjBuild() { lj_release(ds, out); }
  uint32_t count_of(uint32_t type) const { return e.interner[type].count; }
  bool has_rows(uint32_t c) const { return c != kNone && info[c].n_edges > 0; }
  uint32_t n_users() const { return count_of(U); }
  uint32_t n_local(uint32_t type) const { return part_local_count(count_of(type), prank, P); }  // (this rank's)
  uint32_t* alloc(size_t bytes) { return lj_alloc(ds, out, bytes); }
  void hash_in(const void* p, size_t bytes) {
    if (!pc.on) return;
    for (size_t i = 0; i < bytes; ++i) hash = (hash ^ static_cast<const unsigned char*>(p)[i]) * 0x100000001b3ull;
  }
  // bytes of the table the commit stage builds: root[nf], then LjMeta[] on a 16-B boundary
  size_t table_bytes() const { return (((size_t)nf * 2 + 15) & ~(size_t)15) + plans.size() * sizeof(LjMeta); }
};

// The walk of one term over the node program: through computed usersets on the same object,
// through usersets and arrows onto others (`far`); hubs end a path. Every (node, near | far) once.
static void walk_term(const LjBuild& b, uint32_t t, std::vector<TermVisit>& out) {
  std::vector<std::pair<uint32_t, bool>> st{{t, false}};
  std::vector<uint8_t> seen(b.nf, 0);
  seen[t] = 1;
  while (!st.empty()) {
    const auto [n, far] = st.back();
    st.pop_back();
    out.push_back({n, kNone, far});
    if (b.hub[n]) continue;
    const DevNode& nd = b.nodes[n];
    for (uint32_t k = 0; k < nd.count; ++k) {
      const DevItem& it = b.items[nd.first + k];
      out.push_back({n, nd.first + k, far});
      uint32_t next = kNone;
      bool nfar = far;
      if (nd.kind == NK_RELATION && it.kind == IT_KIND && it.srel != kEllipsis) next = it.target, nfar = true;
      else if (nd.kind == NK_UNION && it.kind == IT_COMPUTED) next = it.target;
      else if (nd.kind == NK_UNION && it.kind == IT_ARROW && it.target != kNoNode) next = it.target, nfar = true;
      if (next < b.nf && !(seen[next] & (nfar ? 2 : 1))) {
        seen[next] |= nfar ? 2 : 1;
        st.push_back({next, nfar});
      }
    }
  }
}

// Does a walk flatten? Unions, computed usersets, arrows and stored relations only, every target a
// forward node. Caveated (or expiring) relationships to direct subjects are the caveat plane of
// the slots; through a userset or an arrow they would condition a whole hub: not flattened.
static bool walk_flattens(const LjBuild& b, const std::vector<TermVisit>& walk) {
  for (const TermVisit& v : walk) {
    const DevNode& nd = b.nodes[v.node];
    if (b.hub[v.node] || nd.kind == NK_NIL) continue;
    if (nd.kind != NK_RELATION && nd.kind != NK_UNION) return false;
    if (v.item == kNone) continue;
    const DevItem& it = b.items[v.item];
    if (nd.kind == NK_RELATION) {
      if (it.kind != IT_KIND || (it.srel != kEllipsis && (b.has_rows(it.csr_ext) || it.target >= b.nf))) return false;
    } else if (it.kind == IT_ARROW) {
      if (b.has_rows(it.csr_ext) || (it.target != kNoNode && it.target >= b.nf)) return false;
    } else if (it.kind != IT_COMPUTED || it.target >= b.nf) {
      return false;  // (IT_SUB: a nested join)
    }
  }
  return true;
}

// What a root's walk reads: the CSRs (direct-subject ones also into dfeed, by whether the root
// reads them on its resource's own object), the hubs it ends at, caveated relationships.
static void plan_reads(LjBuild& b, LabelPlan& pl, std::vector<uint32_t>& hubs_all) {
  for (const TermVisit& v : pl.walk) {
    const DevNode& nd = b.nodes[v.node];
    if (v.item == kNone) {
      if (b.hub[v.node]) hubs_all.push_back(v.node);
      continue;
    }
    const DevItem& it = b.items[v.item];
    if (nd.kind == NK_RELATION) {
      const bool direct = it.srel == kEllipsis;
      pl.cav |= b.has_rows(it.csr_ext);
      for (uint32_t c : {it.csr_plain, it.csr_ext}) {
        if (!b.has_rows(c)) continue;
        b.csrs_all.push_back(c);
        if (!direct) continue;
        b.dfeed.push_back(c);
        b.dfeed_type.push_back({c, nd.type});
        if (v.far) b.remote.insert(c);
        else b.own_roots[c].push_back(pl.p);
      }
    } else if (nd.kind == NK_UNION && it.kind == IT_ARROW && it.target != kNoNode && b.has_rows(it.csr_plain)) {
      b.csrs_all.push_back(it.csr_plain);
    }
  }
}

// 1. hubs, the subject type, and the roots: permissions whose operands flatten. False: no label join.
static bool lj_stage_plan(LjBuild& b) {
  const Schema& sc = *b.e.schema;
  const uint32_t nf = b.nf, R = (uint32_t)sc.rels.size();
  // hubs: targets of usersets and arrows that are unions of stored subjects and usersets of hubs
  find_hubs(b.nodes, b.items, nf, [&](uint32_t i) { return b.has_rows(b.items[i].csr_ext); }, b.hub, b.loc);
  if (b.P > 1)  // a partitioned graph replicates the hierarchy of the schema's hubs only
    for (uint32_t h = 0; h < nf; ++h) b.hub[h] &= h < b.e.part_hub_node.size() ? b.e.part_hub_node[h] : 0;
  // the subject type: the most common direct subject type of the stored relations
  std::vector<uint64_t> by_type(sc.types.size(), 0);
  for (uint32_t n = 0; n < nf; ++n)
    if (b.nodes[n].kind == NK_RELATION)
      for (uint32_t k = 0; k < b.nodes[n].count; ++k) {
        const DevItem& it = b.items[b.nodes[n].first + k];
        if (it.kind == IT_KIND && it.srel == kEllipsis && it.csr_plain != kNone) by_type[it.stype] += b.info[it.csr_plain].n_edges;
      }
  b.U = (uint32_t)(std::max_element(by_type.begin(), by_type.end()) - by_type.begin());
  if (by_type.empty() || by_type[b.U] == 0) return false;
  std::vector<uint32_t> hubs_all;
  for (uint32_t p = 0; p < nf && p < R && p < 0xFFFFu; ++p) {
    const DevNode& nd = b.nodes[p];
    LabelPlan pl;
    pl.p = p;
    if (b.hub[p]) {  // a hub root (group#member@user): its own vertex is the only V, no slot
      hubs_all.push_back(p);
      b.plans.push_back(std::move(pl));
      continue;
    }
    if (!sc.rels[p].is_perm) continue;
    if (nd.kind == NK_EXCLUDE || nd.kind == NK_INTERSECT) {
      if (nd.count > (uint32_t)kLjTerms) continue;
      for (uint32_t k = 0; k < nd.count; ++k) {
        pl.terms.push_back(b.items[nd.first + k].target);
        if (nd.kind == NK_EXCLUDE && k > 0) pl.neg |= (uint8_t)(1u << k);
      }
    } else if (nd.kind == NK_UNION || nd.kind == NK_RELATION) {
      pl.terms.push_back(p);
    } else {
      continue;
    }
    if (std::any_of(pl.terms.begin(), pl.terms.end(), [&](uint32_t t) { return t >= nf; })) continue;
    for (uint32_t t : pl.terms) walk_term(b, t, pl.walk);
    if (!walk_flattens(b, pl.walk)) continue;
    plan_reads(b, pl, hubs_all);
    b.plans.push_back(std::move(pl));
  }
  if (b.plans.empty()) return false;
  // the root table must fit the join's LDS copy of it
  if (b.table_bytes() > kLjLdsBytes) return false;
  // nothing to gain where the closure join already answers every root the labels would (a
  // partitioned engine needs them: its checks go through the partitioned label join)
  if (!b.ds.cj_host.empty() && !b.e.part_set) {
    bool all_cj = true;
    for (const LabelPlan& pl : b.plans)
      all_cj &= pl.p * 2 + 1 < b.ds.cj_host.size() && reinterpret_cast<const uint16_t*>(b.ds.cj_host.data())[pl.p] != 0xFFFFu;
    if (all_cj) return false;
  }
  // the hubs the roots reach, closed over the hubs' usersets
  // (hierarchy edges are read on the host; the subjects the hubs list directly stay on the device)
  b.used.assign(nf, 0);
  for (size_t k = 0; k < hubs_all.size(); ++k) {
    const uint32_t h = hubs_all[k];
    if (b.used[h]) continue;
    b.used[h] = 1;
    for (uint32_t n : b.loc[h])
      for (uint32_t j = 0; j < b.nodes[n].count; ++j) {
        const DevItem& it = b.items[b.nodes[n].first + j];
        if (it.srel == kEllipsis) continue;
        if (b.has_rows(it.csr_plain)) b.csrs_all.push_back(it.csr_plain);
        hubs_all.push_back(it.target);
      }
  }
  std::sort(b.csrs_all.begin(), b.csrs_all.end());
  b.csrs_all.erase(std::unique(b.csrs_all.begin(), b.csrs_all.end()), b.csrs_all.end());
  std::sort(b.dfeed.begin(), b.dfeed.end());
  b.dfeed.erase(std::unique(b.dfeed.begin(), b.dfeed.end()), b.dfeed.end());
  b.pc.mark("plans");
  return true;
}

// Takes the previous snapshot's tables over whole, under this build's keys. (The arrays pass at
// publish: the current snapshot keeps them, and its checks keep running, until the new one
// replaces it — engine.hip device_publish.)
static void lj_adopt(LjBuild& b) {
  const LjTables& old = b.e.dev->lj;
  b.ds.lj = old;
  b.ds.lj.key = b.key;
  b.ds.lj.dkey = b.dkey;
  b.ds.lj.hgt = b.hkey;
  b.ds.adopt_h.insert(b.ds.adopt_h.end(), old.ptrs.begin(), old.ptrs.end());
  b.ds.bytes += old.bytes;
}

// 2. what the tables depend on: the CSRs read (and the hubs' direct-subject ones), the roots'
// heights and the object counts. A Watch batch that changed none of them keeps the previous
// snapshot's tables; one that changed only direct grants (`dfeed`: the users listed in resource
// slots) keeps them too, and marks the subjects it changed (lj_dirty_path). False: tables adopted.
static bool lj_stage_keys(LjBuild& b) {
  std::vector<uint32_t> all = b.csrs_all, hroots;
  for (uint32_t h = 0; h < b.nf; ++h)
    if (b.used[h])
      for (uint32_t n : b.loc[h])
        for (uint32_t j = 0; j < b.nodes[n].count; ++j) {
          const DevItem& it = b.items[b.nodes[n].first + j];
          if (b.nodes[n].kind == NK_RELATION && it.srel == kEllipsis && it.stype == b.U && b.has_rows(it.csr_plain))
            all.push_back(it.csr_plain);
        }
  std::sort(all.begin(), all.end());
  all.erase(std::unique(all.begin(), all.end()), all.end());
  for (uint32_t c : all) {
    std::vector<uint64_t>& k = std::binary_search(b.dfeed.begin(), b.dfeed.end(), c) ? b.dkey : b.key;
    k.insert(k.end(), {c, (uint64_t)(uintptr_t)b.table[c].nbr, b.info[c].n_edges, b.table[c].n_rows});
  }
  for (const LabelPlan& pl : b.plans) {
    b.key.push_back(pl.p);
    b.hkey.push_back(pl.p < b.ds.hgt.size() ? b.ds.hgt[pl.p] : nullptr);
    hroots.push_back(pl.p);
  }
  for (const TypeInterner& ti : b.e.interner) b.key.push_back(ti.count);
  b.key.push_back(b.max_depth);
  const DeviceSnapshot* old = b.e.dev && !b.e.dev->lj.host.empty() ? b.e.dev : nullptr;
  if (old && old->lj.key == b.key && old->lj.dkey == b.dkey && old->lj.hgt == b.hkey) {
    lj_adopt(b);
    return false;
  }
  // the direct-grant CSRs every root reads on its resource's own object only
  std::vector<uint32_t> own_only;
  for (auto& [c, v] : b.own_roots) {
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    if (!b.remote.count(c)) own_only.push_back(c);
  }
  const char* why = "";
  if (old && old->lj.key == b.key && lj_dirty_path(b.e, b.ds, b.dkey, b.hkey, b.max_depth, own_only, hroots, why)) {
    lj_adopt(b);
    lj_mark_dirty(b.e, b.ds, b.dkey, b.own_roots);
    b.pc.mark("dirty");
    return false;
  }
  if (b.pc.on && old) b.pc.line += std::string(" rebuild=\"") + (old->lj.key == b.key ? why : "structure") + "\"";
  return true;
}

// 3. host copies of every CSR the flattening and the hierarchy read
static void lj_stage_host_rows(LjBuild& b) {
  for (uint32_t c : b.csrs_all) {
    const DevCSR& t = b.table[c];
    HostRows& h = b.rows[c];
    h.n_rows = t.n_rows;
    h.off.resize((size_t)h.n_rows + 1);
    HIP_OK(hipMemcpy(h.off.data(), t.off, h.off.size() * 4, hipMemcpyDeviceToHost));
    h.nbr.resize(b.info[c].n_edges);
    if (!h.nbr.empty()) HIP_OK(hipMemcpy(h.nbr.data(), t.nbr, h.nbr.size() * 4, hipMemcpyDeviceToHost));
    if (t.is_ext && !h.nbr.empty()) {
      h.cav.resize(h.nbr.size());
      h.exp.resize(h.nbr.size());
      HIP_OK(hipMemcpy(h.cav.data(), t.cav, h.cav.size() * 4, hipMemcpyDeviceToHost));
      HIP_OK(hipMemcpy(h.exp.data(), t.exp_us, h.exp.size() * 8, hipMemcpyDeviceToHost));
    }
  }
  b.pc.mark("host_copies");
}

// Does some hub list the wildcard among its direct subjects?
static bool lj_hub_lists_wildcard(const LjBuild& b) {
  std::vector<void*> tmp;
  unsigned hw = 0;
  try {
    unsigned* flag = dalloc<unsigned>(tmp, 1);
    HIP_OK(hipMemset(flag, 0, 4));
    for (auto& [c, base] : b.dsrc)
      hipLaunchKernelGGL(k_any_wildcard, dim3(grid_for(b.info[c].n_edges)), dim3(kBlock), 0, 0, b.table[c].nbr,
                         (unsigned long long)b.info[c].n_edges, flag);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpy(&hw, flag, 4, hipMemcpyDeviceToHost));
  } catch (...) {
    free_list(tmp);
    throw;
  }
  free_list(tmp);
  return hw != 0;
}

// 4. the hierarchy: one vertex per object of every hub used, x -> y when x lists y#h'; its tree
// labels and covers. False: too many vertices, or a hub that lists the wildcard.
static bool lj_stage_hierarchy(LjBuild& b) {
  const uint32_t nf = b.nf;
  b.base.assign(nf, 0);
  uint64_t nv64 = 0;
  for (uint32_t h = 0; h < nf; ++h)
    if (b.used[h]) b.base[h] = nv64, nv64 += b.count_of(b.nodes[h].type);
  if (nv64 >= (1ull << 31)) return false;
  const uint32_t NV = b.NV = (uint32_t)nv64;
  std::vector<std::pair<uint32_t, uint32_t>> edges;  // (parent, child)
  for (uint32_t h = 0; h < nf; ++h) {
    if (!b.used[h]) continue;
    const uint32_t nh = b.count_of(b.nodes[h].type);
    for (uint32_t n : b.loc[h]) {
      if (b.nodes[n].kind != NK_RELATION) continue;
      for (uint32_t j = 0; j < b.nodes[n].count; ++j) {
        const DevItem& it = b.items[b.nodes[n].first + j];
        if (!b.has_rows(it.csr_plain)) continue;
        if (it.srel == kEllipsis) {
          if (it.stype == b.U) b.dsrc.push_back({it.csr_plain, b.base[h]});  // (other types never match a U check)
          continue;
        }
        const HostRows& hr = b.rows.at(it.csr_plain);
        const uint32_t nt = b.count_of(b.nodes[it.target].type);
        for (uint32_t x = 0; x < hr.n_rows && x < nh; ++x)
          for (uint32_t q = hr.off[x]; q < hr.off[x + 1]; ++q) {
            const uint32_t y = hr.nbr[q];
            if (y < nt) edges.push_back({(uint32_t)(b.base[h] + x), (uint32_t)(b.base[it.target] + y)});
          }
      }
    }
  }
  b.pc.mark("edges");
  std::vector<uint32_t> poff((size_t)NV + 1, 0), pnbr(edges.size()), coff((size_t)NV + 1, 0), cnbr(edges.size());
  for (auto& ed : edges) ++poff[ed.second + 1], ++coff[ed.first + 1];
  for (uint32_t v = 0; v < NV; ++v) poff[v + 1] += poff[v], coff[v + 1] += coff[v];
  {
    std::vector<uint32_t> pa(poff.begin(), poff.end() - 1), ca(coff.begin(), coff.end() - 1);
    for (auto& ed : edges) pnbr[pa[ed.second]++] = ed.first, cnbr[ca[ed.first]++] = ed.second;
  }
  edges.clear();
  edges.shrink_to_fit();
  uint32_t n_cyclic = 0;
  hier_labels_any(NV, poff, pnbr, coff, cnbr, b.lab, b.cov_off, b.cov_pre, n_cyclic);
  // a hub root's vertices at or above the depth budget are deferred (the end word's top bit)
  for (const LabelPlan& pl : b.plans) {
    if (!pl.terms.empty()) continue;
    b.any_hub_root = true;
    const uint32_t p = pl.p;
    if (p < b.ds.hgt.size() && b.ds.hgt[p] && b.ds.hcount[p]) {
      std::vector<uint32_t> hh(b.ds.hcount[p]);
      HIP_OK(hipMemcpy(hh.data(), b.ds.hgt[p], hh.size() * 4, hipMemcpyDeviceToHost));
      const uint32_t nh = b.count_of(b.nodes[p].type);
      for (uint32_t x = 0; x < nh; ++x)
        if (x >= hh.size() || hh[x] >= b.max_depth) b.lab[2 * (b.base[p] + x) + 1] |= kLjDeep;
    }
  }
  b.bits = NV < (1u << 24) - 1u ? 24u : 32u;
  // a hub that lists the wildcard holds every subject: not labelled
  if (lj_hub_lists_wildcard(b)) return false;
  b.pc.mark("hierarchy");
  return true;
}

// 4b. the arrow forest (a dirty subject's checks, k_label_join round 2): the objects a
// resource's flattening visits are those its arrows and non-hub usersets lead to; when every
// object leads to at most one other (a document's folder, a folder's parent) they form a forest,
// and the grants flattened into R's slot are those of R and its ancestors. Preorder intervals
// over it let the join test "X is R or an ancestor of R" in one compare: a changed grant of the
// subject on X touches R's slot only then. No forest (an object with two such edges, a cycle, a
// partitioned graph): a dirty subject's checks defer, as before.
static void lj_stage_forest(LjBuild& b) {
  const size_t n_types = b.e.schema->types.size();
  b.af_base.assign(n_types, kNone);
  b.af_rows.assign(n_types, 0);
  if (b.P != 1) return;
  struct Trav {
    uint32_t csr;
    uint16_t src, dst;
  };
  std::vector<Trav> trav;  // the arrows and non-hub usersets the roots' walks cross
  std::vector<char> vtype(n_types, 0);
  for (const LabelPlan& pl : b.plans) {
    if (pl.terms.empty()) continue;
    vtype[b.nodes[pl.p].type] = 1;
    for (const TermVisit& v : pl.walk) {
      if (v.item == kNone) continue;
      const DevNode& nd = b.nodes[v.node];
      const DevItem& it = b.items[v.item];
      const bool crosses = (nd.kind == NK_UNION && it.kind == IT_ARROW) ||
                           (nd.kind == NK_RELATION && it.kind == IT_KIND && it.srel != kEllipsis);
      if (crosses && it.target < b.nf && !b.hub[it.target] && b.has_rows(it.csr_plain))
        trav.push_back({it.csr_plain, nd.type, b.nodes[it.target].type});
    }
  }
  for (const Trav& tv : trav) vtype[tv.src] = vtype[tv.dst] = 1;
  uint64_t nva = 0;
  for (size_t t = 0; t < vtype.size(); ++t)
    if (vtype[t]) b.af_base[t] = (uint32_t)nva, b.af_rows[t] = b.count_of((uint32_t)t), nva += b.af_rows[t];
  bool forest = nva > 0 && nva < (1ull << 31);
  std::vector<uint32_t>& par = b.par;
  if (forest) par.assign(nva, kNone), b.via.assign(nva, kNone);
  std::sort(trav.begin(), trav.end(), [](const Trav& x, const Trav& y) { return x.csr < y.csr; });
  trav.erase(std::unique(trav.begin(), trav.end(), [](const Trav& x, const Trav& y) { return x.csr == y.csr; }), trav.end());
  for (const Trav& tv : trav) {
    if (!forest) break;
    const HostRows& hr = b.rows.at(tv.csr);
    const uint32_t nx = std::min(hr.n_rows, b.af_rows[tv.src]), ny = b.af_rows[tv.dst];
    for (uint32_t x = 0; x < nx && forest; ++x)
      for (uint32_t q = hr.off[x]; q < hr.off[x + 1]; ++q) {
        const uint32_t y = hr.nbr[q];
        if (y == kWildcard || y >= ny) continue;
        const uint32_t v = b.af_base[tv.src] + x, p = b.af_base[tv.dst] + y;
        if (v == p || (par[v] != kNone && par[v] != p)) {
          forest = false;
          break;
        }
        par[v] = p;
        b.via[v] = tv.csr;
      }
  }
  if (forest) {  // preorder over the children, from every parentless vertex
    const uint32_t NVa = (uint32_t)nva;
    std::vector<uint32_t> coff2((size_t)NVa + 1, 0), cn2;
    for (uint32_t v = 0; v < NVa; ++v)
      if (par[v] != kNone) ++coff2[par[v] + 1];
    for (uint32_t v = 0; v < NVa; ++v) coff2[v + 1] += coff2[v];
    cn2.resize(coff2[NVa]);
    {
      std::vector<uint32_t> at(coff2.begin(), coff2.end() - 1);
      for (uint32_t v = 0; v < NVa; ++v)
        if (par[v] != kNone) cn2[at[par[v]]++] = v;
    }
    b.af_lab.assign(2 * (size_t)NVa, 0);
    uint32_t ctr = 0, done = 0;
    std::vector<std::pair<uint32_t, uint32_t>> stk;  // (vertex, next child)
    for (uint32_t r0 = 0; r0 < NVa; ++r0) {
      if (par[r0] != kNone) continue;
      stk.push_back({r0, coff2[r0]});
      b.af_lab[2 * (size_t)r0] = ctr++;
      while (!stk.empty()) {
        auto& [v, c] = stk.back();
        if (c < coff2[v + 1]) {
          const uint32_t ch = cn2[c++];
          b.af_lab[2 * (size_t)ch] = ctr++;
          stk.push_back({ch, coff2[ch]});
        } else {
          b.af_lab[2 * (size_t)v + 1] = ctr;
          ++done;
          stk.pop_back();
        }
      }
    }
    if (done != NVa) forest = false;  // (a cycle: vertices no root reaches)
  }
  if (!forest) {
    b.af_lab.clear();
    par.clear();
    b.via.clear();
    std::fill(b.af_base.begin(), b.af_base.end(), kNone);
  }
  if (b.pc.on) b.pc.line += std::string(" forest=") + (forest ? std::to_string(nva) : "none");
}

// 5. Flattens term t of resource r: the users it reaches without entering a hub, the hub vertices
// it enters (as label intervals), a wildcard; f.over: not representable, the resource is deferred.
static void lj_flatten(const LjBuild& b, uint32_t r, uint32_t t, Flat& f, std::vector<uint64_t>& stack,
                       std::vector<uint64_t>& seen) {
  const uint32_t U = b.U;
  f.D.clear();
  f.V.clear();
  f.C.clear();
  f.wild = f.over = false;
  stack.assign(1, ((uint64_t)t << 32) | r);
  seen.clear();
  while (!stack.empty()) {
    const uint64_t s = stack.back();
    stack.pop_back();
    const uint32_t n = (uint32_t)(s >> 32), x = (uint32_t)s;
    if (b.hub[n]) {
      if (x < b.count_of(b.nodes[n].type)) f.V.push_back((uint32_t)(b.base[n] + x));
      if (f.V.size() > kLjFlatCap) return f.over = true, void();
      continue;
    }
    if (b.P > 1 && part_owner(x, b.P) != b.prank) return f.over = true, void();  // another rank's rows
    if (std::find(seen.begin(), seen.end(), s) != seen.end()) continue;
    seen.push_back(s);
    if (seen.size() > 256) return f.over = true, void();  // (a long arrow chain: the bundles walk it)
    const DevNode& nd = b.nodes[n];
    for (uint32_t k = 0; k < nd.count; ++k) {
      const DevItem& it = b.items[nd.first + k];
      if (nd.kind == NK_UNION && it.kind == IT_COMPUTED) {
        stack.push_back(((uint64_t)it.target << 32) | x);
        continue;
      }
      if (nd.kind == NK_RELATION && it.srel == kEllipsis && it.stype == U && b.has_rows(it.csr_ext)) {
        // caveated / expiring direct subjects: a caveat decided by the stored context alone is a
        // plain edge or none (Engine::caveat_static); a partial one a caveated pair; an expiring
        // relationship is for the bundles (its visibility depends on the check's time)
        const HostRows& hx = b.rows.at(it.csr_ext);
        if (x < hx.n_rows)
          for (uint32_t q = hx.off[x]; q < hx.off[x + 1]; ++q) {
            if (hx.exp[q] != 0) return f.over = true, void();
            const uint32_t y = hx.nbr[q], cv = hx.cav[q];
            const uint8_t st = cv < b.e.caveat_static.size() ? b.e.caveat_static[cv] : (uint8_t)cel::PARTIAL;
            if (st == cel::FALSE) continue;
            if (st == cel::TRUE) {
              if (y == kWildcard) f.wild = true;
              else f.D.push_back(y);
            } else {
              f.C.push_back(y == kWildcard ? kLjCavWild : y);
              f.C.push_back(cv);
            }
          }
        if (f.C.size() > 2 * kLjFlatCap) return f.over = true, void();
      }
      if (!b.has_rows(it.csr_plain) || (nd.kind == NK_UNION && (it.kind != IT_ARROW || it.target == kNoNode))) continue;
      const HostRows& hr = b.rows.at(it.csr_plain);
      if (x >= hr.n_rows) continue;
      for (uint32_t q = hr.off[x]; q < hr.off[x + 1]; ++q) {
        const uint32_t y = hr.nbr[q];
        if (nd.kind == NK_RELATION && it.srel == kEllipsis) {
          if (it.stype != U) break;
          if (y == kWildcard) f.wild = true;
          else f.D.push_back(y);
        } else if (y != kWildcard) {
          stack.push_back(((uint64_t)it.target << 32) | y);
        }
      }
      if (f.D.size() > kLjFlatCap || stack.size() > 16 * kLjFlatCap) return f.over = true, void();
    }
  }
  std::sort(f.D.begin(), f.D.end());
  f.D.erase(std::unique(f.D.begin(), f.D.end()), f.D.end());
  if (!f.C.empty()) {  // caveated pairs once each (kept beside a plain grant of the same user:
                       // the check still evaluates the caveat, which may fail)
    std::vector<std::pair<uint32_t, uint32_t>> cp;
    for (size_t q = 0; q < f.C.size(); q += 2) cp.push_back({f.C[q], f.C[q + 1]});
    std::sort(cp.begin(), cp.end());
    cp.erase(std::unique(cp.begin(), cp.end()), cp.end());
    f.C.clear();
    for (auto& [u, cv] : cp) f.C.push_back(u | kLjCav), f.C.push_back(cv);
  }
  // V as intervals, nested ones dropped (an interval inside another adds nothing)
  std::vector<std::pair<uint32_t, uint32_t>> iv;
  for (uint32_t v : f.V) iv.push_back({b.lab[2 * (size_t)v] & ~kSlotOverflow, b.lab[2 * (size_t)v + 1] & ~kLjDeep});
  std::sort(iv.begin(), iv.end(), [](auto& x, auto& y) { return x.first < y.first || (x.first == y.first && x.second > y.second); });
  f.V.clear();
  uint32_t reach = 0;
  bool any = false;
  for (auto& [lo, hi] : iv) {
    if (any && hi <= reach) continue;
    f.V.push_back(lo);
    f.V.push_back(hi - lo);
    reach = hi;
    any = true;
  }
}

// Flattens every term of a root over resource r; false: some term is not representable.
static bool lj_flatten_terms(const LjBuild& b, const LabelPlan& pl, uint32_t r, std::vector<Flat>& fs,
                             std::vector<uint64_t>& stack, std::vector<uint64_t>& seen) {
  bool over = false;
  for (size_t t = 0; t < pl.terms.size(); ++t) lj_flatten(b, r, pl.terms[t], fs[t], stack, seen), over |= fs[t].over;
  return !over;
}

// The words a resource's flattened terms take as one inline slot, in 24-bit fields or whole
// words; inline_ok: every term's counts fit the header.
static uint32_t lj_slot_words(const std::vector<Flat>& fs, bool& inline_ok, bool p24) {
  uint32_t fields = 0;
  inline_ok = true;
  for (const Flat& f : fs) {
    fields += (uint32_t)(f.D.size() + f.C.size() + f.V.size());
    inline_ok &= f.D.size() + f.C.size() <= kLjMaxD && f.V.size() / 2 <= kLjMaxV;
  }
  return p24 ? (32u + 24u * fields + 31u) / 32u : 1u + fields;
}

// The slot width and the encoding from a sample of every root's resources: 16 words when nearly
// every resource fits, else 32; 24-bit fields only where they buy something — a narrower slot,
// or clearly fewer extension records (their decoding costs ALU per entry: config 3, whose
// records fit 16 words either way, ran 7 % slower packed). Also per root its heights (a resource
// at or above the budget is deferred). False: the slots would take more than half of the free HBM.
static bool lj_stage_sizing(LjBuild& b) {
  b.hgt_host.resize(b.plans.size());
  for (size_t k = 0; k < b.plans.size(); ++k) {
    const uint32_t p = b.plans[k].p;
    if (b.plans[k].terms.empty() || !(p < b.ds.hgt.size() && b.ds.hgt[p] && b.ds.hcount[p])) continue;
    b.hgt_host[k].resize(b.ds.hcount[p]);
    HIP_OK(hipMemcpy(b.hgt_host[k].data(), b.ds.hgt[p], (size_t)b.ds.hcount[p] * 4, hipMemcpyDeviceToHost));
  }
  // inline slots of 24-bit fields (LjEnt24) when every entry fits: users (below the caveated-pair
  // flag when a root has caveated pairs), hierarchy preorder numbers and lengths, caveat instances
  bool any_cav = false;
  for (const LabelPlan& pl : b.plans) any_cav |= pl.cav;
  const bool can_pack = b.NV < 0xFFFFFFu && b.n_users() < (any_cav ? 0x7FFFFFu : 0xFFFFFFu) &&
                        b.e.caveat_static.size() < 0xFFFFFFu;
  uint32_t sw32 = 16, sw24 = 16;
  uint64_t n_all = 0, ext32 = 0, ext24 = 0;
  for (LabelPlan& pl : b.plans) {
    if (pl.terms.empty()) continue;
    const uint32_t n_res = b.n_local(b.nodes[pl.p].type);
    const uint32_t n_samp = std::min<uint32_t>(n_res, 4096);
    uint32_t fit32 = 0, fit24 = 0;
    std::vector<std::pair<uint32_t, uint32_t>> wds;  // (words unpacked, packed) of the inline ones
    std::vector<Flat> fs(pl.terms.size());
    std::vector<uint64_t> st, seen;
    for (uint32_t k = 0; k < n_samp; ++k) {
      const uint32_t r = (uint32_t)(((uint64_t)k * 2654435761ull) % std::max<uint32_t>(n_res, 1)) * b.P + b.prank;
      if (!lj_flatten_terms(b, pl, r, fs, st, seen)) continue;
      bool ok;
      const uint32_t w32 = lj_slot_words(fs, ok, false), w24 = lj_slot_words(fs, ok, true);
      if (!ok) {
        ++ext32, ++ext24, ++n_all;
        continue;
      }
      fit32 += w32 <= 16, fit24 += w24 <= 16;
      wds.push_back({w32, w24});
      ++n_all;
    }
    const uint32_t need32 = fit32 >= n_samp - n_samp / 32 ? 16u : 32u;
    const uint32_t need24 = fit24 >= n_samp - n_samp / 32 ? 16u : 32u;
    for (auto& [w32, w24] : wds) ext32 += w32 > need32, ext24 += w24 > need24;
    pl.sw_need = need32;
    sw32 = std::max(sw32, need32);
    sw24 = std::max(sw24, need24);
  }
  // packed when it removes extension records (config 2: 3 % -> 0.15 % of the resources), or
  // narrows the slot without adding them (config 3 at 16 words: 0.01 % -> 0.3 %, and a wave waits
  // for its slowest lane's extra round trip — 9.0 vs 9.9 G checks/s unpacked)
  b.pack = can_pack && ((ext24 + n_all / 50 < ext32) || (sw24 < sw32 && ext24 <= ext32 + n_all / 1000));
  if (const char* f = debug_env("GCK_DEBUG_LJ_PACK")) b.pack = can_pack && atoi(f) != 0;  // (an A/B of the encoding)
  b.sw = b.pack ? sw24 : sw32;
  if (b.pc.on)
    b.pc.line += " sample[n=" + std::to_string(n_all) + " ext32=" + std::to_string(ext32) + " ext24=" + std::to_string(ext24) +
                 " sw32=" + std::to_string(sw32) + " sw24=" + std::to_string(sw24) + "]";
  // memory: every root's slots plus the user slots must take at most half of the free HBM
  uint64_t need = (uint64_t)b.n_local(b.U) * kUSlotWords * 4;
  for (const LabelPlan& pl : b.plans)
    if (!pl.terms.empty()) need += (uint64_t)b.n_local(b.nodes[pl.p].type) * b.sw * 4;
  size_t free_b = 0, total_b = 0;
  HIP_OK(hipMemGetInfo(&free_b, &total_b));
  if (need > free_b / 2) return false;
  b.pc.mark("sizing");
  return true;
}

// User slots over the hierarchy (closure.inc k_user_slots_1p: the covers of the vertices listing
// each subject, inline or as a list), and the hierarchy's labels on the device.
static void lj_stage_user_slots(LjBuild& b) {
  const uint32_t n_users = b.n_users();
  std::vector<void*> tmp;
  try {
    // (kept with the snapshot when a hub root reads its vertex's interval from it)
    // (+64 B: k_label_join loads kLines - 1 lines from a hub root's label line, and the second
    // one of the array's last line would lie past the end)
    uint32_t* d_lab = b.any_hub_root ? b.alloc(std::max<size_t>(b.lab.size(), 1) * 4 + 64)
                                     : dalloc<uint32_t>(tmp, std::max<size_t>(b.lab.size(), 1));
    if (b.any_hub_root) HIP_OK(hipMemset(d_lab + b.lab.size(), 0, 64));
    b.lab_dev = d_lab;
    uint32_t* d_coff = dalloc<uint32_t>(tmp, b.cov_off.size());
    uint32_t* d_cpre = dalloc<uint32_t>(tmp, std::max<size_t>(b.cov_pre.size(), 1));
    // subject -> the vertices listing it, a CSR over the subject type built on the device from
    // every hub's direct-subject CSRs: counts, scan, scatter with each hub's vertex base
    uint64_t n_pairs = 0;
    for (auto& [c, base] : b.dsrc) n_pairs += b.info[c].n_edges;
    if (n_pairs >= (1ull << 32)) throw Error(GCK_E_CAPACITY, "label join: too many direct memberships");
    const uint32_t nu = b.n_local(b.U);  // the subjects whose slots this rank holds
    uint32_t* d_doff = dalloc<uint32_t>(tmp, (size_t)nu + 1);
    uint32_t* d_dnbr = dalloc<uint32_t>(tmp, std::max<uint64_t>(n_pairs, 1));
    uint32_t* d_cnt = dalloc<uint32_t>(tmp, std::max<uint32_t>(nu, 1));
    HIP_OK(hipStreamSynchronize(nullptr));
    b.hash_in(b.lab.data(), b.lab.size() * 4);
    if (!b.lab.empty()) HIP_OK(hipMemcpy(d_lab, b.lab.data(), b.lab.size() * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_coff, b.cov_off.data(), b.cov_off.size() * 4, hipMemcpyHostToDevice));
    if (!b.cov_pre.empty()) HIP_OK(hipMemcpy(d_cpre, b.cov_pre.data(), b.cov_pre.size() * 4, hipMemcpyHostToDevice));
    // (a partitioned graph: the subjects this rank owns, at their part_local index)
    HIP_OK(hipMemset(d_cnt, 0, (size_t)std::max<uint32_t>(nu, 1) * 4));
    for (auto& [c, base] : b.dsrc)
      hipLaunchKernelGGL(k_count_subjects_part, dim3(grid_for(b.info[c].n_edges)), dim3(kBlock), 0, 0, b.table[c].nbr,
                         (unsigned long long)b.info[c].n_edges, n_users, b.prank, b.P, d_cnt);
    HIP_OK(hipGetLastError());
    device_excl_scan(d_cnt, nu, d_doff);
    HIP_OK(hipMemcpy(d_cnt, d_doff, (size_t)std::max<uint32_t>(nu, 1) * 4, hipMemcpyDeviceToDevice));
    for (auto& [c, base] : b.dsrc)
      hipLaunchKernelGGL(k_transpose_scatter_base, dim3(grid_for(b.info[c].n_edges)), dim3(kBlock), 0, 0, b.table[c].off,
                         b.table[c].nbr, b.table[c].n_rows, (unsigned long long)b.info[c].n_edges, n_users, d_cnt, d_dnbr,
                         (uint32_t)base, b.prank, b.P);
    HIP_OK(hipGetLastError());
    uint32_t* s = b.alloc((size_t)std::max<uint32_t>(nu, 1) * kUSlotWords * 4);
    // (bidir.inc build_user_slots; the sizing has already bounded the slots, and the lists are
    // allocated whatever is free)
    if (nu)
      b.ulist = build_user_slots(b.bits, d_doff, d_dnbr, nu, d_lab, d_coff, d_cpre, b.NV, s, [&](size_t bytes) { return b.alloc(bytes); }).list;
    b.uslot = s;
  } catch (...) {
    free_list(tmp);
    throw;
  }
  free_list(tmp);
  b.pc.mark("user_slots");
}

// The arrow forest on the device: its labels, the parent edges for the chain walk (tupleset CSR
// << 32 | parent), and each vertex's ancestors in one line (lj_chain_wave: its whole chain in one
// round).
static void lj_stage_forest_upload(LjBuild& b) {
  if (b.af_lab.empty()) return;
  const std::vector<uint32_t>& par = b.par;
  auto upload = [&](const void* src, size_t bytes) {
    b.hash_in(src, bytes);
    uint32_t* q = b.alloc(std::max<size_t>(bytes, 1));
    if (bytes) HIP_OK(hipMemcpy(q, src, bytes, hipMemcpyHostToDevice));
    return q;
  };
  b.out.af = upload(b.af_lab.data(), b.af_lab.size() * 4);
  std::vector<unsigned long long> afp(par.size());
  for (size_t v = 0; v < par.size(); ++v) afp[v] = ((unsigned long long)b.via[v] << 32) | par[v];
  b.out.afp = reinterpret_cast<unsigned long long*>(upload(afp.data(), afp.size() * 8));
  b.out.afp_n = (uint32_t)par.size();
  std::vector<uint32_t> anc(par.size() * kAncWords, 0u);
  host_parallel(par.size(), 1 << 14, [&](size_t lo, size_t hi) {
    for (size_t v = lo; v < hi; ++v) {
      uint32_t* L = &anc[v * kAncWords];
      uint32_t n = 0, x = (uint32_t)v;
      while (par[x] != kNone) {
        if (n + 1 == kAncWords) {
          n |= kAncOver;
          break;
        }
        x = par[x];
        L[++n] = x;
      }
      L[0] = n;
    }
  });
  b.out.anc = upload(anc.data(), anc.size() * 4);
}

// One resource's slot from its flattened terms. Inline when the counts fit the header and the
// entries fit w[0, sw) (zeroed): the header, then the entries as words or as 24-bit fields. Else
// an extension header in w and the record appended to `ext` (w[1]: where it begins there).
// True: inline.
static bool lj_encode_slot(const std::vector<Flat>& fs, uint32_t sw, bool pack, uint32_t* w, std::vector<uint32_t>& ext) {
  bool ok;
  const uint32_t words = lj_slot_words(fs, ok, pack);
  if (!ok || words > sw) {
    w[0] = kLjHdrExt;
    w[1] = (uint32_t)ext.size();
    uint32_t h0 = (uint32_t)fs.size();
    for (size_t t = 0; t < fs.size(); ++t) h0 |= (fs[t].wild ? 1u : 0u) << (8 + t);
    ext.push_back(h0);
    for (const Flat& f : fs) ext.push_back((uint32_t)(f.D.size() + f.C.size())), ext.push_back((uint32_t)(f.V.size() / 2));
    for (const Flat& f : fs) {
      ext.insert(ext.end(), f.D.begin(), f.D.end());
      ext.insert(ext.end(), f.C.begin(), f.C.end());
      ext.insert(ext.end(), f.V.begin(), f.V.end());
    }
    return false;
  }
  uint32_t hdr = 0, pos = 1, fld = 0;
  // a 24-bit field at bit 32 + 24 j of the slot (the caveated-pair flag and wildcard
  // re-encoded: LjEnt24)
  auto put24 = [&](uint32_t v) {
    const uint32_t bit = 32u + 24u * fld++, i = bit >> 5, sh = bit & 31u;
    w[i] |= v << sh;
    if (sh > 8u) w[i + 1] |= v >> (32u - sh);
  };
  for (size_t t = 0; t < fs.size(); ++t) {
    const Flat& f = fs[t];
    const uint32_t nD = (uint32_t)(f.D.size() + f.C.size());
    hdr |= (nD | (uint32_t)(f.V.size() / 2) << 5 | (f.wild ? 1u : 0u) << 9) << (10 * t);
    if (pack) {
      for (uint32_t v : f.D) put24(v);
      for (size_t q = 0; q < f.C.size(); q += 2) {
        const uint32_t a = f.C[q];
        put24(a == (kLjCav | kLjCavWild) ? 0xFFFFFFu : ((a & ~kLjCav) | LjEnt24::kCav));
        put24(f.C[q + 1]);
      }
      for (uint32_t v : f.V) put24(v);
    } else {
      for (uint32_t v : f.D) w[pos++] = v;
      for (uint32_t v : f.C) w[pos++] = v;
      for (uint32_t v : f.V) w[pos++] = v;
    }
  }
  w[0] = hdr;
  return true;
}

// 5b. the chain program of a root (LjChain, lj_chain_walk): per term the sets of schema nodes its
// flattening holds at each depth of the resource's forest chain — the nodes reached through
// computed usersets on one object, then through the level's arrow on the parent — and the
// direct-user classes those nodes read. Exact only where the walk can follow the flattening: every
// arrow of a level over one tupleset CSR (the forest edge the walk checks), no userset to a node
// that is not a hub (its objects would be other chains), unions and stored relations only.
// Otherwise (false) the root has no program and its overlay hits defer, as before.
// (Its closure follows computed usersets only, from several nodes at once: not walk_term, whose
// visits cross arrows and usersets.)
static bool lj_chain_of(const LjBuild& b, const LabelPlan& pl, LjChain& ch) {
  const uint32_t nf = b.nf;
  std::memset(&ch, 0, sizeof(ch));
  std::memset(ch.first, kLjChainEnd, sizeof(ch.first));
  std::vector<std::vector<uint32_t>> sets;
  auto closure = [&](std::vector<uint32_t> st) {
    std::vector<char> seen(nf, 0);
    std::vector<uint32_t> out;
    while (!st.empty()) {
      const uint32_t n = st.back();
      st.pop_back();
      if (n >= nf || seen[n] || b.hub[n]) continue;
      seen[n] = 1;
      out.push_back(n);
      const DevNode& nd = b.nodes[n];
      if (nd.kind != NK_UNION) continue;
      for (uint32_t k = 0; k < nd.count; ++k)
        if (b.items[nd.first + k].kind == IT_COMPUTED) st.push_back(b.items[nd.first + k].target);
    }
    std::sort(out.begin(), out.end());
    return out;
  };
  for (size_t t = 0; t < pl.terms.size(); ++t) {
    std::vector<uint32_t> N = closure({pl.terms[t]});
    uint8_t* link = &ch.first[t];
    for (;;) {
      const auto f = std::find(sets.begin(), sets.end(), N);
      if (f != sets.end()) {
        *link = (uint8_t)(f - sets.begin());
        break;
      }
      if (sets.size() == kLjChainLvls) return false;
      LjChainLvl L{};
      L.arrow = 0xFFFFu;
      L.next = kLjChainEnd;
      uint32_t type = kNone, arrow = kNone;
      std::vector<uint32_t> targets;
      for (uint32_t n : N) {
        const DevNode& nd = b.nodes[n];
        if (type != kNone && nd.type != type) return false;
        type = nd.type;
        if (nd.kind == NK_NIL) continue;
        if (nd.kind != NK_RELATION && nd.kind != NK_UNION) return false;
        for (uint32_t k = 0; k < nd.count; ++k) {
          const DevItem& it = b.items[nd.first + k];
          if (nd.kind == NK_RELATION) {
            if (it.kind != IT_KIND) return false;
            if (it.srel != kEllipsis) {
              if (it.target == kNoNode || it.target >= nf || !b.hub[it.target]) return false;
              continue;  // (a hub's members: the slot's intervals)
            }
            if (it.stype != b.U) continue;
            for (uint32_t c : {it.csr_plain, it.csr_ext})
              if (b.has_rows(c)) {
                if (L.n == kLjChainCls || c >= 0xFFFFu) return false;
                L.csr[L.n++] = (uint16_t)c;
              }
          } else if (it.kind == IT_ARROW) {
            if (it.target == kNoNode || it.target >= nf || b.hub[it.target] || !b.has_rows(it.csr_plain)) continue;
            if (arrow != kNone && arrow != it.csr_plain) return false;
            arrow = it.csr_plain;
            targets.push_back(it.target);
          } else if (it.kind != IT_COMPUTED) {
            return false;
          }
        }
      }
      if (type == kNone || type >= b.af_base.size() || b.af_base[type] == kNone || (arrow != kNone && arrow >= 0xFFFFu)) return false;
      L.af_base = b.af_base[type];
      const size_t idx = sets.size();
      sets.push_back(N);
      ch.lvl[idx] = L;
      *link = (uint8_t)idx;
      if (targets.empty()) break;
      ch.lvl[idx].arrow = (uint16_t)arrow;
      link = &ch.lvl[idx].next;
      N = closure(targets);
    }
  }
  for (size_t t = 0; t < pl.terms.size(); ++t)
    if (ch.first[t] >= sets.size()) return false;
  for (size_t l = 0; l < sets.size(); ++l)
    if (ch.lvl[l].next != kLjChainEnd && ch.lvl[l].next >= sets.size()) return false;
  return true;
}

// The slots of root k over this rank's resources, in parallel, and its extension records (those
// that do not fit inline). False: more extension words than a slot can address.
static bool lj_root_slots(LjBuild& b, size_t k, std::vector<uint32_t>& slots, std::vector<uint32_t>& ext_all) {
  const LabelPlan& pl = b.plans[k];
  const uint32_t sw = b.sw, P = b.P, prank = b.prank;
  // (a partitioned graph: the resources this rank owns, slot li = resource li * P + rank)
  const uint32_t n_loc = b.n_local(b.nodes[pl.p].type);
  slots.assign((size_t)std::max<uint32_t>(n_loc, 1) * sw, 0);
  std::mutex ext_mu;
  std::vector<std::pair<uint32_t, std::vector<uint32_t>>> exts;  // (first slot of the chunk, records)
  std::atomic<uint64_t> n_ext{0}, n_over{0}, n_pairs{0};  // (GCK_DEBUG_PHASES: the slot formats)
  const std::vector<uint32_t>& hh = b.hgt_host[k];
  host_parallel(n_loc, 4096, [&](size_t lo, size_t hi) {
    std::vector<Flat> fs(pl.terms.size());
    std::vector<uint64_t> st, seen;
    std::vector<uint32_t> ext;  // (offsets in it are chunk-local; made global below)
    for (size_t li = lo; li < hi; ++li) {
      const size_t r = li * P + prank;
      uint32_t* w = &slots[li * sw];
      if (!hh.empty() && (r >= hh.size() || hh[r] >= b.max_depth)) {
        w[0] = kLjHdrOverflow;
      } else if (!lj_flatten_terms(b, pl, (uint32_t)r, fs, st, seen)) {
        w[0] = kLjHdrOverflow;
        ++n_over;
      } else {
        for (const Flat& f : fs) n_pairs += f.C.size() / 2;
        if (!lj_encode_slot(fs, sw, b.pack, w, ext)) ++n_ext;
      }
    }
    std::lock_guard<std::mutex> lk(ext_mu);
    exts.push_back({(uint32_t)lo, std::move(ext)});
  });
  if (b.pc.on)
    b.pc.line += " root" + std::to_string(pl.p) + "[n=" + std::to_string(n_loc) + " need=" + std::to_string(pl.sw_need) +
                 " ext=" + std::to_string(n_ext.load()) +
                 " deferred=" + std::to_string(n_over.load()) + " pairs=" + std::to_string(n_pairs.load()) + "]";
  std::sort(exts.begin(), exts.end(), [](auto& x, auto& y) { return x.first < y.first; });
  for (size_t c = 0; c < exts.size(); ++c) {
    const uint32_t lo = exts[c].first, hi = c + 1 < exts.size() ? exts[c + 1].first : n_loc;
    const uint32_t at = (uint32_t)ext_all.size();
    if (ext_all.size() + exts[c].second.size() >= (1ull << 31)) return false;
    for (uint32_t r = lo; r < hi; ++r)
      if (slots[(size_t)r * sw] == kLjHdrExt) slots[(size_t)r * sw + 1] += at;
    ext_all.insert(ext_all.end(), exts[c].second.begin(), exts[c].second.end());
  }
  return true;
}

// Resource slots and the LjMeta of every root; a hub root's "slot" is its vertex's interval in the
// labels. False: lj_root_slots refused.
static bool lj_stage_res_slots(LjBuild& b) {
  auto upload = [&](const void* src, size_t bytes) {
    b.hash_in(src, bytes);
    uint32_t* q = b.alloc(bytes);
    HIP_OK(hipMemcpy(q, src, bytes, hipMemcpyHostToDevice));
    return q;
  };
  b.root.assign(b.nf, 0xFFFFu);
  for (size_t k = 0; k < b.plans.size(); ++k) {
    const LabelPlan& pl = b.plans[k];
    LjMeta M{};
    M.uslot = b.uslot;
    M.ulist = b.ulist;
    M.u_rows = b.n_users();
    M.r_rows = b.count_of(b.nodes[pl.p].type);
    M.rtype = b.nodes[pl.p].type;
    M.utype = (uint16_t)b.U;
    M.n_terms = (uint8_t)pl.terms.size();
    b.root[pl.p] = (uint16_t)b.metas.size();
    if (pl.terms.empty()) {  // hub root
      M.rslot = b.lab_dev + 2 * b.base[pl.p];
      b.metas.push_back(M);
      continue;
    }
    std::vector<uint32_t> slots, ext_all;
    if (!lj_root_slots(b, k, slots, ext_all)) return false;
    M.rslot = upload(slots.data(), slots.size() * 4);
    M.rext = ext_all.empty() ? nullptr : upload(ext_all.data(), ext_all.size() * 4);
    M.neg = pl.neg;
    M.cav = pl.cav ? 1 : 0;
    M.pack = b.pack ? 1 : 0;
    M.apre = b.out.af && b.af_base[M.rtype] != kNone ? b.out.af + 2 * (size_t)b.af_base[M.rtype] : nullptr;
    if (M.apre && b.out.afp) {
      LjChain ch;
      if (lj_chain_of(b, pl, ch)) M.chain = reinterpret_cast<LjChain*>(upload(&ch, sizeof(LjChain)));
      if (b.pc.on) {
        b.pc.line += std::string(" chain") + std::to_string(pl.p) + "=";
        if (!M.chain) b.pc.line += "no";
        for (size_t t = 0; M.chain && t < pl.terms.size(); ++t) b.pc.line += "t" + std::to_string(ch.first[t]);
        for (uint32_t l = 0; M.chain && l < kLjChainLvls && (ch.lvl[l].n || ch.lvl[l].arrow); ++l)
          b.pc.line += "[" + std::to_string(ch.lvl[l].af_base) + "," + std::to_string(ch.lvl[l].n) + "," +
                       std::to_string(ch.lvl[l].arrow) + "," + std::to_string(ch.lvl[l].next) + "]";
      }
    }
    b.metas.push_back(M);
  }
  b.pc.mark("res_slots");
  return true;
}

// The root table, and the tables into the snapshot.
static void lj_stage_commit(LjBuild& b) {
  std::vector<unsigned char> blob;
  auto put = [&](const void* src, size_t bytes) {
    const size_t o = (blob.size() + 15) & ~(size_t)15;
    blob.resize(o + bytes);
    std::memcpy(blob.data() + o, src, bytes);
    return (uint32_t)o;
  };
  b.hash_in(b.root.data(), b.root.size() * 2);
  put(b.root.data(), b.root.size() * 2);
  b.out.o_meta = put(b.metas.data(), b.metas.size() * sizeof(LjMeta));
  if (blob.size() != b.table_bytes()) throw Error(GCK_E_DEVICE, "engine invariant violated: label root table size");
  // the closure join keeps the stage when it answers every root the labels answer (config 4's
  // tuned path); the labels take it when they cover every closure-join root and more
  bool covers = true, more = false;
  for (uint32_t p = 0; p < b.nf; ++p) {
    const bool in_cj = !b.ds.cj_host.empty() && p * 2 + 1 < b.ds.cj_host.size() &&
                       reinterpret_cast<const uint16_t*>(b.ds.cj_host.data())[p] != 0xFFFFu;
    const bool in_lj = b.root[p] != 0xFFFFu;
    covers &= !in_cj || in_lj;
    more |= in_lj && !in_cj;
  }
  LjTables& t = b.out;
  t.preferred = covers && more;
  for (const LabelPlan& pl : b.plans) t.cav |= pl.cav;
  t.host = std::move(blob);
  t.sw = b.sw;
  t.bits = b.bits;
  t.key = std::move(b.key);
  t.dkey = std::move(b.dkey);
  t.hgt = std::move(b.hkey);
  t.users = b.n_users();
  t.af_base = std::move(b.af_base);
  t.af_rows = std::move(b.af_rows);
  std::sort(b.dfeed_type.begin(), b.dfeed_type.end());
  b.dfeed_type.erase(std::unique(b.dfeed_type.begin(), b.dfeed_type.end()), b.dfeed_type.end());
  t.dtype = std::move(b.dfeed_type);
  if (b.pc.on) {
    char h[32];
    snprintf(h, sizeof(h), " hash=%016llx", (unsigned long long)b.hash);
    b.pc.line += " sw=" + std::to_string(b.sw) + " bits=" + std::to_string(b.bits) + " pack=" + (b.pack ? "24" : "32") + h;
  }
  b.ds.lj = std::move(t);
  t = LjTables{};  // (nothing left to free)
}

// Builds the label join's tables for the snapshot into ds.lj, or leaves it empty when no permission
// qualifies or a stage refuses. Runs after build_bidir (heights are known; the closure join, when
// the snapshot has one of its roots, keeps the stage: the two are not combined).
static void build_labels(Engine& e, DeviceSnapshot& ds, const std::vector<DevNode>& nodes,
                         const std::vector<DevItem>& items, const std::vector<DevCSR>& table,
                         const std::vector<CsrInfo>& info) {
  if (e.cfg.flags & (GCK_FLAG_NO_LABELS | GCK_FLAG_NO_SLOTS)) return;
  LjBuild b{e, ds, nodes, items, table, info, e.part_world, e.part_rank, ds.n_fwd, e.cfg.max_depth ? e.cfg.max_depth : 50};
  if (!lj_stage_plan(b)) return;       // no root, too many for the LDS table, or all the closure join's
  if (!lj_stage_keys(b)) return;       // the previous snapshot's tables adopted
  lj_stage_host_rows(b);
  if (!lj_stage_hierarchy(b)) return;  // >= 2^31 vertices, or a hub lists the wildcard
  lj_stage_forest(b);
  if (!lj_stage_sizing(b)) return;     // more than half of the free HBM
  lj_stage_user_slots(b);              // (the first allocation: from here `b.out` owns arrays)
  lj_stage_forest_upload(b);
  if (!lj_stage_res_slots(b)) return;  // >= 2^31 extension words in one root
  lj_stage_commit(b);
}
