// hs_host.cpp -- see hs_host.hpp.  Host logic only: parsing, formatting, planes, evaluation; every
// number on the search path is computed on the GPU behind include/hsearch.h.
#include "hs_host.hpp"

#include <errno.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <sys/types.h>

#include <algorithm>
#include <fstream>
#include <functional>
#include <limits>
#include <map>
#include <random>
#include <sstream>
#include <thread>
#include <unordered_map>
#include <unordered_set>

#include "../../include/hs_tables.h"
#include "../../include/hsearch.h"
#include "../../include/hsearch_dist.h"

namespace hsearch {

Planes DrawPlanes(uint32_t dim, uint32_t K, uint32_t L, double W, uint32_t seed) {
  Planes p;
  p.dim = dim;
  p.K = K;
  p.L = L;
  p.W = W;
  p.a.resize((size_t)L * K * dim);
  p.b.resize((size_t)L * K);
  for (uint32_t l = 0; l < L; ++l) {
    // one engine and one pair of distributions per table, as one LSH object owns them
    std::default_random_engine generator(seed + l);
    std::normal_distribution<double> normal(0.0, 1.0);
    std::uniform_real_distribution<double> width(0, W);
    for (uint32_t k = 0; k < K; ++k) {
      double* row = &p.a[((size_t)l * K + k) * dim];
      for (uint32_t i = 0; i < dim; ++i) row[i] = normal(generator);
      p.b[(size_t)l * K + k] = width(generator);
    }
  }
  return p;
}

bool ReadPointsFile(const std::string& path, uint32_t dim, std::vector<std::string>* names,
                    std::vector<Point>* points) {
  std::ifstream fin(path.c_str());
  if (!fin) return false;
  std::string line;
  while (std::getline(fin, line)) {
    names->push_back(line);
    std::getline(fin, line);
    std::istringstream iss(line);
    Point point;
    point.data.assign(dim, 0.0);
    for (uint32_t i = 0; i < dim; ++i) iss >> point.data[i];
    points->push_back(point);
  }
  return true;
}

bool PointsToCodes(const std::vector<Point>& pts, uint32_t dim, std::vector<double>* table,
                   std::vector<uint8_t>* codes, std::string* err) {
  const uint32_t k = dim / 8;
  table->clear();
  codes->assign(pts.size() * (size_t)k, 0);
  struct Row {
    uint64_t w[8];
    bool operator<(const Row& o) const { return memcmp(w, o.w, sizeof(w)) < 0; }
  };
  std::map<Row, uint8_t> rows;  // exact bit patterns: the GPU must hash the very same doubles
  for (size_t i = 0; i < pts.size(); ++i) {
    if (pts[i].data.size() != dim) {
      if (err) *err = "DB point with the wrong dimension";
      return false;
    }
    for (uint32_t p = 0; p < k; ++p) {
      Row r;
      memcpy(r.w, &pts[i].data[8 * p], 64);
      std::map<Row, uint8_t>::iterator it = rows.find(r);
      if (it == rows.end()) {
        if (rows.size() >= 32) {
          if (err)
            *err = "DB points are not embeddings over an alphabet of <= 32 residues; the GPU index "
                   "stores the DB as residue codes (arbitrary-point DBs are not supported)";
          return false;
        }
        const uint8_t code = (uint8_t)rows.size();
        it = rows.insert(std::make_pair(r, code)).first;
        table->insert(table->end(), &pts[i].data[8 * p], &pts[i].data[8 * p] + 8);
      }
      (*codes)[i * k + p] = it->second;
    }
  }
  if (table->empty()) table->assign(8, 0.0);
  return true;
}

namespace {

struct SearchHits {
  std::vector<uint32_t> q, id, table;
  std::vector<double> dist;
  uint64_t n = 0;
};
struct HandleCloser {
  hs_handle* h;
  ~HandleCloser() { hs_destroy(h); }
};

// how the rank threads exchange hits (SetShardTransport) and what a rank holds (SetShardPartition)
ShardTransport g_shard_transport = kTransportRccl;
ShardPartition g_shard_partition = kPartitionQueries;
// T extra probes per table of the running Search / SearchSharded call (hs_set_multiprobe)
uint32_t g_probes = 0;

// Cost of every table for the table-partitioned layout, from a sample of the DB's k-mers: the sum over the
// table's buckets of (sample k-mers in the bucket)^2 -- for queries distributed like the DB, proportional to
// the (member, query) pairs the table contributes to the join.  One short-lived handle with all L planes (no
// index) hashes the sample; buckets are told apart by the fingerprint of their K ints (a collision would only
// nudge an estimate).  Empty on any failure: the caller then deals the tables round robin.
std::vector<double> TableCosts(hs_params prm, const Planes& planes, const double* coords, const uint8_t* sample,
                               uint64_t n_sample, int device) {
  std::vector<double> cost;
  if (!sample || n_sample < 64) return cost;
  hs_handle* h = nullptr;
  prm.device = device;
  if (hs_create(&prm, planes.a.data(), planes.b.data(), coords, &h) != HS_OK) {
    hs_destroy(h);
    return cost;
  }
  HandleCloser closer = {h};
  std::vector<int32_t> ints((size_t)n_sample * prm.L * prm.K);
  if (hs_hash_codes(h, sample, n_sample, ints.data()) != HS_OK) return cost;
  cost.assign(prm.L, 0.0);
  std::vector<uint64_t> fp(n_sample);
  for (uint32_t l = 0; l < prm.L; ++l) {
    for (uint64_t i = 0; i < n_sample; ++i) fp[i] = hs_key_fingerprint(&ints[((size_t)i * prm.L + l) * prm.K], prm.K, 0);
    std::sort(fp.begin(), fp.end());
    for (uint64_t i = 0, j; i < n_sample; i = j) {
      for (j = i + 1; j < n_sample && fp[j] == fp[i]; ++j) {}
      cost[l] += (double)(j - i) * (double)(j - i);
    }
  }
  return cost;
}


// The device part of Search(): index build (through `build`, on a fresh handle) and the query loop,
// on one GPU (devices.size() == 1 and !sharded: hs_query, no communicator) or query-sharded over
// several: one host thread and one handle per GPU, the index built on every GPU, rank
// r searching its contiguous block of centres, hits all-gathered over RCCL (hs_comm_query) so that
// every rank -- rank 0 writes the file -- holds all hits in the reference's order.
// qcodes != null: the centres are k-mers of the handle's coordinate table, given as residue codes
// [nq][k]; they cross PCIe as k bytes each (hs_query_codes) and `flat` is unused.
// annotate: `out` receives, instead of the hits, per DB k-mer reached its nearest centre in ascending id (the rule
// of hs_annotate, include/hsearch.h).  One GPU: hs_annotate, no hit list anywhere.  Query blocks over several
// GPUs: every rank annotates its block, nothing is exchanged between them, and the ranks' lists -- query numbers
// made global -- are merged by hs_merge_best.  Table and bucket partitions gather the hits as before; the gathered
// list is reduced by hs_merge_best.

// hs_annotate into `out` through the two-call pattern (a first capacity of 1 / 64 of the index)
hs_status AnnotateInto(hs_handle* h, const double* flat, const uint8_t* qcodes, uint64_t nq, double R,
                       const double* radii, SearchHits* out) {
  hs_index_info info;
  hs_status st = hs_index_info_get(h, &info);
  if (st != HS_OK) return st;
  uint64_t cap = std::max<uint64_t>(1024, info.n / 64);
  for (;;) {
    out->q.resize(cap);
    out->id.resize(cap);
    out->table.resize(cap);
    out->dist.resize(cap);
    st = hs_annotate(h, qcodes ? nullptr : flat, qcodes, nq, R, radii, out->id.data(), out->q.data(),
                     out->table.data(), out->dist.data(), cap, &out->n);
    if (st != HS_ERR_CAPACITY) return st;
    cap = out->n;
  }
}

// hs_merge_best over the first in.n tuples of `in`
hs_status MergeBestInto(const SearchHits& in, SearchHits* out) {
  out->q.resize(in.n);
  out->id.resize(in.n);
  out->table.resize(in.n);
  out->dist.resize(in.n);
  return hs_merge_best(in.id.data(), in.q.data(), in.table.data(), in.dist.data(), in.n, out->id.data(),
                       out->q.data(), out->table.data(), out->dist.data(), in.n, &out->n);
}

int RunSearch(hs_params prm, const Planes& planes, const double* coords,
              const std::function<hs_status(hs_handle*, uint32_t rank)>& build, const double* flat,
              const uint8_t* qcodes, uint64_t nq, double R, const std::vector<int>& devices, bool sharded,
              SearchHits* out, std::string* err, std::vector<uint64_t>* table_sizes,
              const uint8_t* db_sample = nullptr, uint64_t n_db_sample = 0, const double* radii = nullptr,
              bool annotate = false, uint32_t topk = 0) {
  const uint32_t world = (uint32_t)devices.size();
  if (!world) {
    if (err) *err = "no device given";
    return HS_ERR_INVALID;
  }
  if (topk && (sharded || annotate)) {  // (the exchange gathers hit lists; an annotation has one line per k-mer)
    if (err)
      *err = sharded ? "top-k hits per centre are not supported together with the multi-GPU exchange"
                     : "top-k hits per centre are not supported together with best_per_position";
    return HS_ERR_INVALID;
  }
  if (radii && sharded) {  // (hs_comm_query* take one radius)
    if (err) *err = "per-centre radii are not supported together with the multi-GPU exchange";
    return HS_ERR_INVALID;
  }
  // table partition: rank r holds the tables tabs[r] (global numbers, ascending) of ALL k-mers
  const bool by_tables = sharded && g_shard_partition == kPartitionTables;
  const bool by_buckets = sharded && g_shard_partition == kPartitionBuckets;
  std::vector<std::vector<uint32_t>> tabs(world);
  if (by_tables) {
    if (world > prm.L) {
      if (err) *err = "table partition: more GPUs than tables";
      return HS_ERR_INVALID;
    }
    const std::vector<double> cost = TableCosts(prm, planes, coords, db_sample, n_db_sample, devices[0]);
    std::vector<uint32_t> owner(prm.L, 0);
    hs_assign_tables(cost.empty() ? nullptr : cost.data(), prm.L, world, owner.data());
    for (uint32_t l = 0; l < prm.L; ++l) tabs[owner[l]].push_back(l);
    if (table_sizes) table_sizes->assign(prm.L, 0);
  }
  const size_t plane_doubles = (size_t)prm.K * 8 * prm.k;
  auto open = [&](int device, hs_handle** h, std::string* msg, uint32_t rank = 0) -> hs_status {
    hs_params p = prm;
    p.device = device;
    hs_status st;
    if (by_tables) {
      std::vector<double> a, b;
      for (uint32_t l : tabs[rank]) {
        a.insert(a.end(), planes.a.begin() + (size_t)l * plane_doubles, planes.a.begin() + (size_t)(l + 1) * plane_doubles);
        b.insert(b.end(), planes.b.begin() + (size_t)l * prm.K, planes.b.begin() + (size_t)(l + 1) * prm.K);
      }
      p.L = (uint32_t)tabs[rank].size();
      st = hs_create(&p, a.data(), b.data(), coords, h);
    } else {
      st = hs_create(&p, planes.a.data(), planes.b.data(), coords, h);
    }
    if (st != HS_OK) {
      *msg = std::string("hs_create: ") + (*h ? hs_last_error(*h) : "no usable gfx950 device");
      hs_destroy(*h);
      *h = nullptr;
    } else if (g_probes && (st = hs_set_multiprobe(*h, g_probes)) != HS_OK) {
      *msg = std::string("hs_set_multiprobe: ") + hs_last_error(*h);
      hs_destroy(*h);
      *h = nullptr;
    }
    return st;
  };
  auto sizes = [&](hs_handle* h) {
    hs_index_info info;
    if (table_sizes && hs_index_info_get(h, &info) == HS_OK)
      table_sizes->assign(info.n_buckets, info.n_buckets + prm.L);
  };
  if (!sharded) {
    hs_handle* h = nullptr;
    std::string msg;
    hs_status st = open(devices[0], &h, &msg);
    if (st != HS_OK) {
      if (err) *err = msg;
      return st;
    }
    HandleCloser closer = {h};
    st = build(h, 0);
    if (st != HS_OK) {
      if (err) *err = std::string("index build: ") + hs_last_error(h);
      return st;
    }
    sizes(h);
    if (annotate) {
      st = AnnotateInto(h, flat, qcodes, nq, R, radii, out);
      if (st != HS_OK && err) *err = std::string("hs_annotate: ") + hs_last_error(h);
      return st;
    }
    if (topk) {  // the rows selected on the device; `out` receives their entries, centre by centre, best first
      std::vector<uint32_t> nn_id((size_t)nq * topk), nn_table((size_t)nq * topk), nn_count(nq);
      std::vector<double> nn_dist((size_t)nq * topk);
      uint64_t n_hits = 0;
      st = hs_query_topk(h, qcodes ? nullptr : flat, qcodes, nq, R, radii, topk, nn_id.data(), nn_table.data(),
                         nn_dist.data(), nn_count.data(), &n_hits);
      if (st != HS_OK) {
        if (err) *err = std::string("hs_query_topk: ") + hs_last_error(h);
        return st;
      }
      for (uint64_t q = 0; q < nq; ++q)
        for (uint32_t r = 0; r < topk && r < nn_count[q]; ++r) {
          out->q.push_back((uint32_t)q);
          out->id.push_back(nn_id[q * topk + r]);
          out->table.push_back(nn_table[q * topk + r]);
          out->dist.push_back(nn_dist[q * topk + r]);
        }
      out->n = out->q.size();
      return HS_OK;
    }
    uint64_t cap = std::max<uint64_t>(1024, 16 * nq);
    for (;;) {
      out->q.resize(cap);
      out->id.resize(cap);
      out->table.resize(cap);
      out->dist.resize(cap);
      if (radii)  // every centre at its own radius
        st = hs_query_radii(h, qcodes ? nullptr : flat, qcodes, nq, radii, out->q.data(), out->id.data(),
                            out->table.data(), out->dist.data(), cap, &out->n, nullptr);
      else
      st = qcodes ? hs_query_codes(h, qcodes, nq, R, out->q.data(), out->id.data(), out->table.data(),
                                   out->dist.data(), cap, &out->n, nullptr)
                  : hs_query(h, flat, nq, R, out->q.data(), out->id.data(), out->table.data(), out->dist.data(),
                             cap, &out->n, nullptr);
      if (st == HS_ERR_CAPACITY) {
        cap = out->n;
        continue;
      }
      break;
    }
    if (st != HS_OK && err) *err = std::string("hs_query: ") + hs_last_error(h);
    return st;
  }
  char cerr[256] = "";
  hs_comm* comm = nullptr;
  hs_status cst = hs_comm_create(g_shard_transport == kTransportLoopback ? HS_COMM_LOOPBACK : HS_COMM_RCCL_LOCAL,
                                 devices.data(), world, &comm, cerr, sizeof(cerr));
  if (cst != HS_OK) {
    if (err) *err = std::string("hs_comm_create: ") + cerr;
    return cst;
  }
  const uint64_t d = 8ull * prm.k;
  std::vector<hs_status> status(world, HS_OK);
  std::vector<std::string> msgs(world);
  std::vector<int> built(world, 0);
  const bool annotate_blocks = annotate && !by_tables && !by_buckets;
  std::vector<SearchHits> rank_rows(annotate_blocks ? world : 0);
  auto rank_main = [&](uint32_t r) {
    hs_handle* h = nullptr;
    hs_status st = open(devices[r], &h, &msgs[r], r);
    HandleCloser closer = {h};
    if (st == HS_OK) {
      st = build(h, r);
      if (st != HS_OK) msgs[r] = std::string("index build: ") + hs_last_error(h);
    }
    if (st == HS_OK && by_tables && table_sizes) {  // (distinct slots per rank)
      hs_index_info info;
      if (hs_index_info_get(h, &info) == HS_OK)
        for (size_t i = 0; i < tabs[r].size(); ++i) (*table_sizes)[tabs[r][i]] = info.n_buckets[i];
    }
    built[r] = st == HS_OK;
    status[r] = st;
    // every rank learns whether all indexes stand before anyone enters the exchange
    hs_comm_barrier(comm, r);
    for (uint32_t x = 0; x < world; ++x)
      if (!built[x]) return;
    if (r == 0 && !by_tables) sizes(h);
    uint64_t lo = 0, hi = 0;
    hs_shard_bounds(nq, world, r, &lo, &hi);
    if (annotate_blocks) {  // this rank's block, annotated; merged below once every rank is done
      SearchHits& rows = rank_rows[r];
      st = AnnotateInto(h, qcodes ? nullptr : flat + lo * d, qcodes ? qcodes + lo * prm.k : nullptr, hi - lo, R, nullptr,
                        &rows);
      if (st != HS_OK) msgs[r] = std::string("hs_annotate: ") + hs_last_error(h);
      for (uint64_t i = 0; st == HS_OK && i < rows.n; ++i) rows.q[i] += (uint32_t)lo;
      status[r] = st;
      return;
    }
    SearchHits mine;  // ranks other than 0 drop theirs
    SearchHits* dst = r == 0 ? out : &mine;
    uint64_t cap = std::max<uint64_t>(1024, 16 * nq);
    for (;;) {  // every rank sees the same total, so every rank repeats (or not) together
      dst->q.resize(cap);
      dst->id.resize(cap);
      dst->table.resize(cap);
      dst->dist.resize(cap);
      hs_handle* hq = h;
#ifdef HS_TEST_HOOKS
      // fault injection (test build of the programs only): this rank enters the exchange having failed
      if (const char* fr = getenv("HS_TEST_FAIL_RANK"))
        if ((uint32_t)atoi(fr) == r) hq = nullptr;
#endif
      if (by_tables)  // every rank passes ALL centres; the merged list comes back (include/hsearch_dist.h)
        st = hs_comm_query_tables(comm, r, hq, tabs[r].data(), (uint32_t)tabs[r].size(), qcodes ? nullptr : flat, qcodes,
                                  nq, R, dst->q.data(), dst->id.data(), dst->table.data(), dst->dist.data(), cap,
                                  &dst->n);
      else if (by_buckets)  // the same, every rank with the whole index and its part of the buckets
        st = hs_comm_query_buckets(comm, r, hq, qcodes ? nullptr : flat, qcodes, nq, R, dst->q.data(), dst->id.data(),
                                   dst->table.data(), dst->dist.data(), cap, &dst->n);
      else
      st = qcodes ? hs_comm_query_codes(comm, r, hq, qcodes + lo * prm.k, hi - lo, (uint32_t)lo, R, dst->q.data(),
                                        dst->id.data(), dst->table.data(), dst->dist.data(), cap, &dst->n)
                  : hs_comm_query(comm, r, hq, flat + lo * d, hi - lo, (uint32_t)lo, R, dst->q.data(),
                                  dst->id.data(), dst->table.data(), dst->dist.data(), cap, &dst->n);
      if (st == HS_ERR_CAPACITY) {
        cap = dst->n;
        continue;
      }
      break;
    }
    if (st != HS_OK) msgs[r] = std::string("hs_comm_query: ") + hs_comm_last_error(comm, r);
    status[r] = st;
  };
  std::vector<std::thread> threads;
  for (uint32_t r = 1; r < world; ++r) threads.emplace_back(rank_main, r);
  rank_main(0);
  for (std::thread& t : threads) t.join();
  hs_comm_destroy(comm);
  for (uint32_t r = 0; r < world; ++r)
    if (status[r] != HS_OK) {
      if (err) *err = "GPU " + std::to_string(devices[r]) + ": " + msgs[r];
      return status[r];
    }
  if (annotate) {
    SearchHits all;
    if (annotate_blocks) {
      for (const SearchHits& rows : rank_rows) {
        all.q.insert(all.q.end(), rows.q.begin(), rows.q.begin() + rows.n);
        all.id.insert(all.id.end(), rows.id.begin(), rows.id.begin() + rows.n);
        all.table.insert(all.table.end(), rows.table.begin(), rows.table.begin() + rows.n);
        all.dist.insert(all.dist.end(), rows.dist.begin(), rows.dist.begin() + rows.n);
        all.n += rows.n;
      }
    } else {
      all.q.swap(out->q);
      all.id.swap(out->id);
      all.table.swap(out->table);
      all.dist.swap(out->dist);
      all.n = out->n;
    }
    const hs_status mst = MergeBestInto(all, out);
    if (mst != HS_OK) {
      if (err) *err = "hs_merge_best failed";
      return mst;
    }
  }
  return HS_OK;
}

// radii (optional argument of the Search functions): one per centre
bool RadiiMatch(const std::vector<double>* radii, size_t n_centers, std::string* err) {
  if (!radii || radii->size() == n_centers) return true;
  if (err) *err = "radii: one radius per centre is needed";
  return false;
}

bool FlattenCenters(const std::vector<Point>& centers, uint32_t dim, std::vector<double>* flat, std::string* err) {
  flat->resize((size_t)centers.size() * dim);
  for (size_t i = 0; i < centers.size(); ++i) {
    if (centers[i].data.size() != dim) {
      if (err) *err = "centre with the wrong dimension";
      return false;
    }
    memcpy(&(*flat)[i * dim], centers[i].data.data(), sizeof(double) * dim);
  }
  return true;
}

}  // namespace

void SetShardTransport(ShardTransport t) { g_shard_transport = t; }
void SetShardPartition(ShardPartition p) { g_shard_partition = p; }

int Search(const std::vector<Point>& kmers, const std::vector<Point>& centers,
           const std::vector<std::string>& kmer_names, const std::vector<std::string>& center_names,
           const uint32_t& hash_K, const uint32_t& hash_L, const double& hash_W,
           const double& hash_R, const std::string& output_file, const Planes& planes, int device,
           std::string* err, std::vector<uint64_t>* table_sizes, uint32_t probes, const std::vector<double>* radii,
           bool best_per_position, uint32_t topk) {
  return SearchSharded(kmers, centers, kmer_names, center_names, hash_K, hash_L, hash_W, hash_R, output_file,
                       planes, std::vector<int>(1, device), false, err, table_sizes, probes, radii,
                       best_per_position, topk);
}

int SearchSharded(const std::vector<Point>& kmers, const std::vector<Point>& centers,
                  const std::vector<std::string>& kmer_names, const std::vector<std::string>& center_names,
                  const uint32_t& hash_K, const uint32_t& hash_L, const double& hash_W,
                  const double& hash_R, const std::string& output_file, const Planes& planes,
                  const std::vector<int>& devices, bool use_comm, std::string* err,
                  std::vector<uint64_t>* table_sizes, uint32_t probes, const std::vector<double>* radii,
                  bool best_per_position, uint32_t topk) {
  if (!RadiiMatch(radii, centers.size(), err)) return HS_ERR_INVALID;
  struct ProbesScope {
    explicit ProbesScope(uint32_t t) { g_probes = t; }
    ~ProbesScope() { g_probes = 0; }
  } probes_scope(probes);
  const uint32_t dim = planes.dim;
  if (dim == 0 || dim % 8 != 0 || planes.K != hash_K || planes.L != hash_L || planes.W != hash_W) {
    if (err) *err = "planes do not match (dim, K, L, W)";
    return HS_ERR_INVALID;
  }
  std::vector<double> table;
  std::vector<uint8_t> codes;
  if (!PointsToCodes(kmers, dim, &table, &codes, err)) return HS_ERR_INVALID;
  std::vector<double> flat;
  if (!FlattenCenters(centers, dim, &flat, err)) return HS_ERR_INVALID;
  hs_params prm;
  memset(&prm, 0, sizeof(prm));
  prm.k = dim / 8;
  prm.K = hash_K;
  prm.L = hash_L;
  prm.W = hash_W;
  prm.alphabet = (uint32_t)(table.size() / 8);
  SearchHits hits;
  const int st = RunSearch(prm, planes, table.data(),
                           [&](hs_handle* h, uint32_t) { return hs_index_build(h, codes.data(), kmers.size()); },
                           flat.data(), nullptr, centers.size(), hash_R, devices, use_comm || devices.size() > 1,
                           &hits, err, table_sizes, codes.data(), std::min<uint64_t>(kmers.size(), 32768),
                           radii ? radii->data() : nullptr, best_per_position, topk);
  if (st != HS_OK) return st;
  std::ofstream fout(output_file.c_str());
  for (uint64_t i = 0; i < hits.n; ++i)  // :240-241; best_per_position: one line per k-mer reached, k-mers ascending
    if (best_per_position)
      fout << kmer_names[hits.id[i]] << " " << center_names[hits.q[i]] << " " << hits.dist[i] << std::endl;
    else
    fout << center_names[hits.q[i]] << " " << kmer_names[hits.id[i]] << " " << hits.dist[i] << std::endl;
  fout.close();
  return HS_OK;
}


bool ReadProteinFasta(const std::string& path, bool ref_compat_eq_swap, ProteinDB* db) {
  std::ifstream fin(path.c_str());
  if (!fin) return false;
  db->name.clear();
  db->start.clear();
  db->residues.clear();
  db->eq_swapped = ref_compat_eq_swap;
  std::string line;
  while (std::getline(fin, line)) {  // protein.hpp:47-66
    if (!line.empty() && line[line.size() - 1] == '\r') line.erase(line.size() - 1);
    if (line.empty()) continue;
    if (line[0] == '>') {
      db->name.push_back(line.substr(1));
      continue;
    }
    db->start.push_back(db->residues.size());
    for (size_t i = 0; i < line.size(); ++i) {
      const char c = line[i];
      int row = (c >= 'A' && c <= 'Z') ? HS_LETTER_TO_CODE[c - 'A'] : -1;
      // the reference keeps AA20[row] and embeds base[] of that letter: rows 5 and 6 trade places
      if (ref_compat_eq_swap && (row == 5 || row == 6)) row = 11 - row;
      db->residues.push_back(row < 0 ? ProteinDB::kUnknown : (uint8_t)row);
    }
  }
  db->start.push_back(db->residues.size());
  return true;
}

// --db-append: the database followed by the sequences of every further one -- sequence numbers and names continue,
// as in the concatenated FASTA file; part_end[i] = where part i ends in the joined residues
static ProteinDB JoinProteinDBs(const ProteinDB& db, const std::vector<ProteinDB>& more, std::vector<uint64_t>* part_end) {
  ProteinDB all = db;
  if (all.start.empty()) all.start.push_back(0);
  all.name.resize(all.start.size() - 1);
  part_end->assign(1, all.residues.size());
  for (const ProteinDB& m : more) {
    const uint64_t base = all.residues.size();
    const size_t n_seq = m.start.empty() ? 0 : m.start.size() - 1;
    for (size_t s = 0; s < n_seq; ++s) {
      all.name.push_back(s < m.name.size() ? m.name[s] : std::string());
      all.start.push_back(base + m.start[s + 1]);
    }
    all.residues.insert(all.residues.end(), m.residues.begin(), m.residues.end());
    part_end->push_back(all.residues.size());
  }
  return all;
}

// The index over the windows of `res` cut into the segments `seg` (seg.size() - 1 of them, ending at res.size()): built
// from the segments of the first part and grown by those of every further part (hs_index_append_windows), which gives
// the index hs_index_build_windows builds over all of them.  Parts end at sequence starts, which are segment starts.
static hs_status BuildWindowsInParts(hs_handle* h, const std::vector<uint8_t>& res, const std::vector<uint64_t>& seg,
                                     const std::vector<uint64_t>& part_end, uint64_t* n_win, uint32_t* win_pos) {
  if (part_end.size() <= 1) return hs_index_build_windows(h, res.data(), res.size(), seg.data(), seg.size() - 1, n_win, win_pos);
  *n_win = 0;
  uint64_t lo = 0;
  size_t at = 0;  // first segment of the part
  for (size_t part = 0; part < part_end.size(); ++part) {
    const uint64_t hi = part_end[part];
    std::vector<uint64_t> local;
    while (at + 1 < seg.size() && seg[at] < hi) local.push_back(seg[at++] - lo);
    local.push_back(hi - lo);
    uint64_t nw = 0;
    uint32_t* const pos = win_pos ? win_pos + *n_win : nullptr;
    const hs_status st = part == 0 ? hs_index_build_windows(h, res.data(), hi, local.data(), local.size() - 1, &nw, pos)
                                   : hs_index_append_windows(h, res.data() + lo, hi - lo, local.data(), local.size() - 1, &nw, pos);
    if (st != HS_OK) return st;
    if (pos)
      for (uint64_t i = 0; i < nw; ++i) pos[i] += (uint32_t)lo;
    *n_win += nw;
    lo = hi;
  }
  return HS_OK;
}

int SearchProteins(const ProteinDB& db, uint32_t kmer_length, const std::vector<Point>& centers,
                   const std::vector<std::string>& center_names, const uint32_t& hash_K,
                   const uint32_t& hash_L, const double& hash_W, const double& hash_R,
                   const std::string& output_file, const Planes& planes, int device, std::string* err,
                   std::vector<uint64_t>* table_sizes, uint64_t* n_windows, bool best_per_position,
                   const std::vector<double>* radii, uint32_t topk, const std::vector<ProteinDB>* more) {
  return SearchProteinsSharded(db, kmer_length, centers, center_names, hash_K, hash_L, hash_W, hash_R,
                               output_file, planes, std::vector<int>(1, device), false, err, table_sizes,
                               n_windows, best_per_position, nullptr, radii, topk, more);
}

int SearchProteinsSharded(const ProteinDB& db_first, uint32_t kmer_length, const std::vector<Point>& centers,
                          const std::vector<std::string>& center_names, const uint32_t& hash_K,
                          const uint32_t& hash_L, const double& hash_W, const double& hash_R,
                          const std::string& output_file, const Planes& planes,
                          const std::vector<int>& devices, bool use_comm, std::string* err,
                          std::vector<uint64_t>* table_sizes, uint64_t* n_windows, bool best_per_position,
                          const std::vector<uint8_t>* center_codes, const std::vector<double>* radii, uint32_t topk,
                          const std::vector<ProteinDB>* more) {
  const uint32_t dim = 8 * kmer_length;
  const bool appended = more && !more->empty();
  if (appended && devices.size() > 1) {
    if (err) *err = "appended databases run on one GPU";
    return HS_ERR_INVALID;
  }
  std::vector<uint64_t> part_end;
  const ProteinDB joined = appended ? JoinProteinDBs(db_first, *more, &part_end) : ProteinDB();
  const ProteinDB& db = appended ? joined : db_first;
  if (!RadiiMatch(radii, centers.size(), err)) return HS_ERR_INVALID;
  if (center_codes && center_codes->size() != centers.size() * (size_t)kmer_length) {
    if (err) *err = "centre codes do not match the centres";
    return HS_ERR_INVALID;
  }
  if (kmer_length == 0 || planes.dim != dim || planes.K != hash_K || planes.L != hash_L ||
      planes.W != hash_W) {
    if (err) *err = "planes do not match (dim, K, L, W)";
    return HS_ERR_INVALID;
  }
  // sequences cut at unknown letters: windows never cross a cut, buffer positions stay the file's
  std::vector<uint8_t> res(db.residues);
  std::vector<uint64_t> seg;
  const size_t n_seq = db.start.empty() ? 0 : db.start.size() - 1;
  for (size_t s = 0; s < n_seq; ++s) {
    seg.push_back(db.start[s]);
    for (uint64_t p = db.start[s]; p < db.start[s + 1]; ++p)
      if (res[p] == ProteinDB::kUnknown) {
        res[p] = 0;
        seg.push_back(p);      // the unknown letter ends a segment ...
        seg.push_back(p + 1);  // ... and forms one of its own (length 1 < k: no window)
      }
  }
  seg.push_back(db.residues.size());
  if (kmer_length == 1) {  // a length-1 segment would be a window: drop the unknown letters' own
    if (err) *err = "kmer length 1 is not supported on a FASTA database";
    return HS_ERR_INVALID;
  }
  std::vector<double> flat;
  if (!FlattenCenters(centers, dim, &flat, err)) return HS_ERR_INVALID;
  hs_params prm;
  memset(&prm, 0, sizeof(prm));
  prm.k = kmer_length;
  prm.K = hash_K;
  prm.L = hash_L;
  prm.W = hash_W;
  prm.alphabet = HS_ALPHABET;
  uint64_t n_win = 0;
  std::vector<uint32_t> win_pos(res.size() + 1);  // there are fewer windows than residues
  SearchHits hits;
  const int rst = RunSearch(
      prm, planes, &HS_AA_COORDS[0][0],
      [&](hs_handle* h, uint32_t rank) {
        uint64_t nw = 0;  // every rank enumerates the same windows; rank 0 keeps their positions
        const hs_status bst = BuildWindowsInParts(h, res, seg, part_end, &nw, rank == 0 ? win_pos.data() : nullptr);
        if (rank == 0) n_win = nw;
        return bst;
      },
      flat.data(), center_codes ? center_codes->data() : nullptr, centers.size(), hash_R, devices,
      use_comm || devices.size() > 1, &hits, err, table_sizes, nullptr, 0, radii ? radii->data() : nullptr,
      best_per_position, topk);
  if (rst != HS_OK) return rst;
  if (n_windows) *n_windows = n_win;
  const uint64_t n_hits = hits.n;
  const std::vector<uint32_t>&hq = hits.q, &hid = hits.id;
  const std::vector<double>& hd = hits.dist;
  // the letter whose embedding is the stored row: with the E <-> Q exchange an input E is shown as
  // Q, which is what the reference's ProteinDB stores and prints
  const char* letters = HS_CODE_TO_LETTER;
  std::ofstream fout(output_file.c_str());
  // best_per_position: the list is the annotation already (kmer_search.cpp:96-121 -- visit order (table, centre),
  // `it2->second.second > dis` replaces -- reduced on the device: hs_annotate), windows ascending
  for (uint64_t i = 0; i < n_hits; ++i) {
    const uint64_t pos = win_pos[hid[i]];
    // sequence of the window: largest s with start[s] <= pos
    const size_t s = (size_t)(std::upper_bound(db.start.begin(), db.start.end() - 1, pos) - db.start.begin()) - 1;
    std::string token;
    if (s < db.name.size()) {
      std::istringstream iss(db.name[s]);
      iss >> token;
    }
    std::string kmer(kmer_length, '?');
    for (uint32_t p = 0; p < kmer_length; ++p) kmer[p] = letters[db.residues[pos + p]];
    if (best_per_position)
      fout << token << "#" << s << "$" << (pos - db.start[s]) << "@" << kmer << "*" << hid[i] << " "
           << center_names[hq[i]] << " " << hd[i] << std::endl;
    else
      fout << center_names[hq[i]] << " " << token << "#" << s << "$" << (pos - db.start[s]) << "@" << kmer
           << "*" << hid[i] << " " << hd[i] << std::endl;
  }
  fout.close();
  return HS_OK;
}

static std::string ProteinLabel(const ProteinDB& db, size_t s);

bool ReadPssmFile(const std::string& path, uint32_t kmer_length, std::vector<std::string>* names,
                  std::vector<double>* S, std::vector<double>* t, std::string* err) {
  std::ifstream fin(path.c_str());
  if (!fin) {
    if (err) *err = "cannot open " + path;
    return false;
  }
  names->clear();
  S->clear();
  t->clear();
  std::map<std::string, int> seen;
  std::string line;
  uint32_t rows_left = 0;
  size_t line_no = 0;
  auto fail = [&](const std::string& what) {
    if (err) *err = path + ":" + std::to_string(line_no) + ": " + what;
    return false;
  };
  auto number = [](const std::string& tok, double* out) {
    char* end = nullptr;
    *out = strtod(tok.c_str(), &end);
    return end != tok.c_str() && *end == 0;
  };
  while (std::getline(fin, line)) {
    ++line_no;
    std::istringstream iss(line);
    std::vector<std::string> tok;
    for (std::string w; iss >> w;) tok.push_back(w);
    if (tok.empty()) continue;
    if (tok[0][0] == '>') {
      if (rows_left) return fail("a profile of fewer than " + std::to_string(kmer_length) + " rows ends here");
      double thr = 0.0;
      if (tok.size() != 2 || tok[0].size() < 2 || !number(tok[1], &thr)) return fail("expected '>name threshold'");
      const std::string name = tok[0].substr(1);
      if (seen[name]++) return fail("profile " + name + " is given twice");
      names->push_back(name);
      t->push_back(thr);
      rows_left = kmer_length;
      continue;
    }
    if (!rows_left) return fail(names->empty() ? "expected '>name threshold'" : "a profile of more rows than the kmer length");
    if (tok.size() != HS_ALPHABET) return fail("expected " + std::to_string(HS_ALPHABET) + " numbers");
    for (const std::string& w : tok) {
      double v = 0.0;
      if (!number(w, &v)) return fail("'" + w + "' is not a number");
      S->push_back(v);
    }
    --rows_left;
  }
  ++line_no;
  if (rows_left) return fail("a profile of fewer than " + std::to_string(kmer_length) + " rows ends here");
  return true;
}

// The windows index every profile call runs on: the database's windows (never across a letter outside the alphabet)
// under the smallest hash family there is -- no hash table takes part in a scan.  win_pos: where every window starts
// in db.residues; id_start [proteins + 1]: the window ids every protein owns.  The caller destroys *h.
static int OpenWindowsIndex(const ProteinDB& db, uint32_t k, int device, hs_handle** h_out, uint64_t* n_win,
                            std::vector<uint32_t>* win_pos, std::vector<uint64_t>* id_start, std::string* err) {
  // sequences cut at unknown letters, as in SearchProteinsSharded: windows never cross a cut
  std::vector<uint8_t> res(db.residues);
  std::vector<uint64_t> seg;
  const size_t n_seq = db.start.empty() ? 0 : db.start.size() - 1;
  std::vector<size_t> first_seg(n_seq + 1);  // the first segment of every protein
  for (size_t s = 0; s < n_seq; ++s) {
    first_seg[s] = seg.size();
    seg.push_back(db.start[s]);
    for (uint64_t p = db.start[s]; p < db.start[s + 1]; ++p)
      if (res[p] == ProteinDB::kUnknown) {
        res[p] = 0;
        seg.push_back(p);
        seg.push_back(p + 1);
      }
  }
  first_seg[n_seq] = seg.size();
  seg.push_back(db.residues.size());
  const Planes planes = DrawPlanes(8 * k, 1, 1, 1.0, 0);
  hs_params prm;
  memset(&prm, 0, sizeof(prm));
  prm.k = k;
  prm.K = 1;
  prm.L = 1;
  prm.W = 1.0;
  prm.alphabet = HS_ALPHABET;
  prm.device = device;
  hs_handle* h = nullptr;
  hs_status st = hs_create(&prm, planes.a.data(), planes.b.data(), &HS_AA_COORDS[0][0], &h);
  *h_out = h;
  if (st != HS_OK) {
    if (err) *err = std::string("hs_create: ") + (h ? hs_last_error(h) : "no usable gfx950 device");
    return st;
  }
  win_pos->assign(res.size() + 1, 0);
  st = hs_index_build_windows(h, res.data(), res.size(), seg.data(), seg.size() - 1, n_win, win_pos->data());
  if (st != HS_OK) {
    if (err) *err = std::string("index build: ") + hs_last_error(h);
    return st;
  }
  // a protein's segments follow one another, so its windows are one id range: the range of its first segment on
  std::vector<uint64_t> seg_ids(seg.size());
  st = hs_window_id_start(seg.data(), seg.size() - 1, k, seg_ids.data());
  if (st != HS_OK) {
    if (err) *err = "hs_window_id_start refused the segments";
    return st;
  }
  id_start->resize(n_seq + 1);
  for (size_t s = 0; s <= n_seq; ++s) (*id_start)[s] = seg_ids[first_seg[s]];
  return HS_OK;
}

// ScanProfiles (topn == 0: every hit at or above t, hs_pssm_scan) and ScanProfilesTopN (topn >= 1: per profile the topn
// best windows at or above t, hs_pssm_topk): the same index, the same lines.  ScanProfilesPerSequence (n_rows_out
// given): the same index, one line per (profile, protein) (hs_pssm_seq_scan).
static int ScanProfilesAny(const ProteinDB& db, uint32_t kmer_length, const std::vector<std::string>& names,
                           const std::vector<double>& S, const std::vector<double>& t, uint32_t topn,
                           const std::string& output_file, int device, std::string* err, uint64_t* n_windows,
                           uint64_t* n_hits_out, uint64_t* n_rows_out = nullptr,
                           const std::vector<double>* pvalue_floor = nullptr) {
  const uint32_t k = kmer_length;
  const size_t nm = t.size();
  if (k < 2 || names.size() != nm || S.size() != nm * (size_t)k * HS_ALPHABET ||
      (pvalue_floor && pvalue_floor->size() != nm)) {
    if (err) *err = k < 2 ? "kmer length 1 is not supported on a FASTA database" : "the profiles do not match the kmer length";
    return HS_ERR_INVALID;
  }
  const size_t n_seq = db.start.empty() ? 0 : db.start.size() - 1;
  hs_handle* h = nullptr;
  uint64_t n_win = 0;
  std::vector<uint32_t> win_pos;
  std::vector<uint64_t> id_start;
  hs_status st = (hs_status)OpenWindowsIndex(db, k, device, &h, &n_win, &win_pos, &id_start, err);
  HandleCloser closer = {h};
  if (st != HS_OK) return st;
  if (n_windows) *n_windows = n_win;
  if (n_rows_out) {
    std::vector<uint32_t> rm, rs, rc, rid, rlo, rhi;
    std::vector<double> rsc;
    uint64_t n_rows = 0, n_hits = 0;
    for (uint64_t cap = 0;;) {  // the row count, then the rows
      for (std::vector<uint32_t>* v : {&rm, &rs, &rc, &rid, &rlo, &rhi}) v->resize(cap);
      rsc.resize(cap);
      st = hs_pssm_seq_scan(h, S.data(), t.data(), nm, id_start.data(), n_seq, rm.data(), rs.data(), rc.data(),
                            rsc.data(), rid.data(), rlo.data(), rhi.data(), cap, &n_rows, &n_hits, nullptr, nullptr);
      if (st == HS_ERR_CAPACITY && n_rows > cap) {
        cap = n_rows;
        continue;
      }
      break;
    }
    if (st != HS_OK) {
      if (err) *err = std::string("hs_pssm_seq_scan: ") + hs_last_error(h);
      return st;
    }
    if (n_hits_out) *n_hits_out = n_hits;
    *n_rows_out = n_rows;
    std::ofstream fout(output_file.c_str());
    char num[64];
    for (uint64_t i = 0; i < n_rows; ++i) {  // offsets are residue offsets in the protein, as the scan's window names
      const size_t s = rs[i];
      const uint64_t at = db.start[s], w0 = id_start[s];
      snprintf(num, sizeof(num), "%.17g", rsc[i]);
      fout << names[rm[i]] << " " << ProteinLabel(db, s) << " " << rc[i] << " " << (win_pos[rid[i]] - at) << " " << num
           << " " << (win_pos[w0 + rlo[i]] - at) << " " << (win_pos[w0 + rhi[i]] - at) << "\n";
    }
    fout.close();
    return HS_OK;
  }
  std::vector<uint32_t> hm, hid;
  std::vector<double> hs;
  uint64_t n_hits = 0;
  if (topn) {  // the rows, selected on the device, flattened into the scan's lists: (profile, rank) order
    std::vector<uint32_t> top_id(nm * (size_t)topn), top_count(nm);
    std::vector<double> top_score(nm * (size_t)topn);
    st = hs_pssm_topk(h, S.data(), t.data(), nm, topn, top_id.data(), top_score.data(), top_count.data(), nullptr);
    if (st != HS_OK) {
      if (err) *err = std::string("hs_pssm_topk: ") + hs_last_error(h);
      return st;
    }
    for (size_t m = 0; m < nm; ++m)
      for (uint32_t r = 0; r < top_count[m]; ++r) {
        hm.push_back((uint32_t)m);
        hid.push_back(top_id[m * topn + r]);
        hs.push_back(top_score[m * topn + r]);
      }
    n_hits = hm.size();
  }
  for (uint64_t cap = 0; !topn;) {  // the hit count, then the hits
    hm.resize(cap);
    hid.resize(cap);
    hs.resize(cap);
    st = hs_pssm_scan(h, S.data(), t.data(), nm, hm.data(), hid.data(), hs.data(), cap, &n_hits, nullptr);
    if (st == HS_ERR_CAPACITY && n_hits > cap) {
      cap = n_hits;
      continue;
    }
    break;
  }
  if (st != HS_OK) {
    if (err) *err = std::string("hs_pssm_scan: ") + hs_last_error(h);
    return st;
  }
  if (n_hits_out) *n_hits_out = n_hits;
  std::vector<double> p_hi;
  if (pvalue_floor && n_hits) {  // the upper end of every hit's p-value under the database's residue composition
    p_hi.resize(n_hits);
    st = hs_pssm_pvalue(h, S.data(), nullptr, pvalue_floor->data(), nm, hm.data(), hs.data(), n_hits, p_hi.data(), nullptr);
    if (st != HS_OK) {
      if (err) *err = std::string("hs_pssm_pvalue: ") + hs_last_error(h);
      return st;
    }
  }
  const char* letters = HS_CODE_TO_LETTER;
  std::ofstream fout(output_file.c_str());
  char num[64], pnum[64];
  for (uint64_t i = 0; i < n_hits; ++i) {
    const uint64_t pos = win_pos[hid[i]];
    const size_t s = (size_t)(std::upper_bound(db.start.begin(), db.start.end() - 1, pos) - db.start.begin()) - 1;
    std::string kmer(k, '?');
    for (uint32_t p = 0; p < k; ++p) kmer[p] = letters[db.residues[pos + p]];
    snprintf(num, sizeof(num), "%.17g", hs[i]);
    fout << names[hm[i]] << " " << ProteinLabel(db, s) << "$" << (pos - db.start[s]) << "@" << kmer << "*" << hid[i]
         << " " << num;
    if (pvalue_floor) {
      snprintf(pnum, sizeof(pnum), "%.17g", p_hi[i]);
      fout << " " << pnum;
    }
    fout << "\n";
  }
  fout.close();
  return HS_OK;
}

int HitPvalues(const ProteinDB& db, uint32_t kmer_length, const std::vector<std::string>& names,
               const std::vector<double>& S, const std::vector<double>& t, const std::vector<double>& t_lo,
               const std::string& output_file, int device, std::string* err, uint64_t* n_windows, uint64_t* n_hits_out) {
  return ScanProfilesAny(db, kmer_length, names, S, t, 0, output_file, device, err, n_windows, n_hits_out, nullptr, &t_lo);
}

int PvalueThresholds(const ProteinDB& db, uint32_t kmer_length, const std::vector<double>& S,
                     const std::vector<double>& p, const std::vector<double>& t_lo, int device,
                     std::vector<double>* t_out, std::vector<double>* p_hi, std::vector<double>* p_lo,
                     std::vector<uint32_t>* flag, std::string* err) {
  const uint32_t k = kmer_length;
  const size_t nm = p.size();
  if (k < 2 || S.size() != nm * (size_t)k * HS_ALPHABET || t_lo.size() != nm) {
    if (err) *err = k < 2 ? "kmer length 1 is not supported on a FASTA database" : "the profiles do not match the kmer length";
    return HS_ERR_INVALID;
  }
  hs_handle* h = nullptr;
  uint64_t n_win = 0;
  std::vector<uint32_t> win_pos;
  std::vector<uint64_t> id_start;
  hs_status st = (hs_status)OpenWindowsIndex(db, k, device, &h, &n_win, &win_pos, &id_start, err);
  HandleCloser closer = {h};
  if (st != HS_OK) return st;
  std::vector<double> hi(nm), lo(nm);
  std::vector<uint32_t> fl(nm);
  t_out->assign(nm, 0.0);
  st = hs_pssm_pvalue_threshold(h, S.data(), nullptr, t_lo.data(), p.data(), nm, t_out->data(), hi.data(), lo.data(),
                                fl.data());
  if (st != HS_OK) {
    if (err) *err = std::string("hs_pssm_pvalue_threshold: ") + hs_last_error(h);
    return st;
  }
  if (p_hi) p_hi->swap(hi);
  if (p_lo) p_lo->swap(lo);
  if (flag) flag->swap(fl);
  return HS_OK;
}

static int FamilyLayoutText(const std::vector<std::string>& names, const std::vector<uint32_t>& hit_x,
                            const std::vector<uint32_t>& hit_y, const std::vector<int32_t>& hit_d, size_t n_hits,
                            std::string* text, std::string* err, uint64_t* n_families, uint64_t* n_conflicts);

int CompareProfiles(uint32_t kmer_length, const std::vector<std::string>& names_x, const std::vector<double>& X,
                    const std::vector<double>& t, const std::vector<std::string>* names_y, const std::vector<double>* Y,
                    uint32_t min_overlap, int columns, const std::string& output_file, int device, std::string* err,
                    uint64_t* n_hits_out, const std::string* families_out, uint64_t* n_families,
                    uint64_t* n_conflicts) {
  const uint32_t k = kmer_length;
  const size_t ka = (size_t)k * HS_ALPHABET, nx = names_x.size(), ny = names_y ? names_y->size() : 0;
  if (k < 1 || X.size() != nx * ka || t.size() != nx || !names_y != !Y || (Y && Y->size() != ny * ka)) {
    if (err) *err = "the profiles do not match the kmer length";
    return HS_ERR_INVALID;
  }
  if (families_out && Y) {
    if (err) *err = "families are laid out from a self comparison only";
    return HS_ERR_INVALID;
  }
  std::vector<double> Xc(X), Yc;
  if (Y) Yc = *Y;
  if (columns >= 0 && (hs_pssm_compare_columns(X.data(), nx, k, HS_ALPHABET, columns, Xc.data()) != HS_OK ||
                       (Y && hs_pssm_compare_columns(Y->data(), ny, k, HS_ALPHABET, columns, Yc.data()) != HS_OK))) {
    if (err) *err = "hs_pssm_compare_columns: a profile entry is NaN, infinite or beyond 2^100";
    return HS_ERR_INVALID;
  }
  const Planes planes = DrawPlanes(8 * k, 1, 1, 1.0, 0);  // (no hash table takes part: the smallest family there is)
  hs_params prm;
  memset(&prm, 0, sizeof(prm));
  prm.k = k;
  prm.K = 1;
  prm.L = 1;
  prm.W = 1.0;
  prm.alphabet = HS_ALPHABET;
  prm.device = device;
  hs_handle* h = nullptr;
  hs_status st = hs_create(&prm, planes.a.data(), planes.b.data(), &HS_AA_COORDS[0][0], &h);
  HandleCloser closer = {h};
  if (st != HS_OK) {
    if (err) *err = std::string("hs_create: ") + (h ? hs_last_error(h) : "no usable gfx950 device");
    return st;
  }
  std::vector<uint32_t> hx, hy;
  std::vector<int32_t> hd;
  std::vector<double> hs;
  uint64_t n_hits = 0, cap = std::max<uint64_t>(1024, 16 * nx);
  for (;;) {
    hx.resize(cap), hy.resize(cap), hd.resize(cap), hs.resize(cap);
    st = hs_pssm_compare(h, Xc.data(), nx, Y ? Yc.data() : nullptr, ny, t.data(), min_overlap, hx.data(), hy.data(),
                         hd.data(), hs.data(), cap, &n_hits, nullptr);
    if (st != HS_ERR_CAPACITY) break;
    cap = n_hits;
  }
  if (st != HS_OK) {
    if (err) *err = std::string("hs_pssm_compare: ") + hs_last_error(h);
    return st;
  }
  std::string families_text;  // laid out before anything is written: a refused layout leaves no output file behind
  if (families_out) {
    const int lst = FamilyLayoutText(names_x, hx, hy, hd, n_hits, &families_text, err, n_families, n_conflicts);
    if (lst != HS_OK) return lst;
  }
  const std::vector<std::string>& ynames = names_y ? *names_y : names_x;
  std::ofstream fout(output_file.c_str());
  char num[64];
  for (uint64_t i = 0; i < n_hits; ++i) {
    snprintf(num, sizeof(num), "%.17g", hs[i]);
    fout << names_x[hx[i]] << " " << ynames[hy[i]] << " " << hd[i] << " " << num << "\n";
  }
  fout.close();
  if (n_hits_out) *n_hits_out = n_hits;
  if (families_out) {
    std::ofstream ffam(families_out->c_str());
    ffam << families_text;
    ffam.close();
  }
  return HS_OK;
}

// the lines of FamilyLayout's file, nothing written yet
static int FamilyLayoutText(const std::vector<std::string>& names, const std::vector<uint32_t>& hit_x,
                            const std::vector<uint32_t>& hit_y, const std::vector<int32_t>& hit_d, size_t n_hits,
                            std::string* text, std::string* err, uint64_t* n_families, uint64_t* n_conflicts) {
  const size_t nm = names.size();
  if (hit_x.size() < n_hits || hit_y.size() < n_hits || hit_d.size() < n_hits) {
    if (err) *err = "the hit lists differ in length";
    return HS_ERR_INVALID;
  }
  std::vector<uint32_t> group(nm), off(nm), order(nm);
  uint64_t groups = 0, conflicts = 0;
  const hs_status st = hs_pssm_family_layout(hit_x.data(), hit_y.data(), hit_d.data(), n_hits, nm, group.data(),
                                             off.data(), order.data(), &groups, &conflicts);
  if (st != HS_OK) {
    if (err)
      *err = "hs_pssm_family_layout: a hit names a profile twice or none, a distance of 2^30 or more, an offset beyond "
             "2^31 - 1 or a family of more than 4096 profiles";
    return st;
  }
  std::vector<uint32_t> first(groups, 0);  // the first profile of every family in the order of the file
  for (size_t i = nm; i-- > 0;) first[group[order[i]]] = order[i];
  std::ostringstream out;
  for (size_t i = 0; i < nm; ++i) {
    const uint32_t m = order[i];
    out << names[first[group[m]]] << " " << names[m] << " " << off[m] << "\n";
  }
  *text = out.str();
  if (n_families) *n_families = groups;
  if (n_conflicts) *n_conflicts = conflicts;
  return HS_OK;
}

int FamilyLayout(const std::vector<std::string>& names, const std::vector<uint32_t>& hit_x,
                 const std::vector<uint32_t>& hit_y, const std::vector<int32_t>& hit_d, const std::string& families_file,
                 std::string* err, uint64_t* n_families, uint64_t* n_conflicts) {
  if (hit_y.size() != hit_x.size() || hit_d.size() != hit_x.size()) {
    if (err) *err = "the hit lists differ in length";
    return HS_ERR_INVALID;
  }
  std::string text;
  const int st = FamilyLayoutText(names, hit_x, hit_y, hit_d, hit_x.size(), &text, err, n_families, n_conflicts);
  if (st != HS_OK) return st;
  std::ofstream fout(families_file.c_str());
  fout << text;
  fout.close();
  return HS_OK;
}

// families numbered in the given order; one that comes back after another is refused
static bool FamilyGroups(const std::vector<std::string>& family, std::vector<uint32_t>* m_group,
                         std::vector<std::string>* fam_names, std::string* err) {
  m_group->resize(family.size());
  for (size_t m = 0; m < family.size(); ++m) {
    if (!m || family[m] != family[m - 1]) {
      if (std::find(fam_names->begin(), fam_names->end(), family[m]) != fam_names->end()) {
        if (err) *err = "the profiles of family " + family[m] + " do not stand next to each other";
        return false;
      }
      fam_names->push_back(family[m]);
    }
    (*m_group)[m] = (uint32_t)fam_names->size() - 1;
  }
  return true;
}

int FamilyScan(const ProteinDB& db, uint32_t kmer_length, const std::vector<std::string>& names,
               const std::vector<double>& S, const std::vector<double>& t, const std::vector<std::string>& family,
               const std::vector<uint32_t>& offset, uint32_t min_blocks, const double* threshold,
               const std::string& output_file, int device, std::string* err, uint64_t* n_windows, uint64_t* n_hits_out,
               uint64_t* n_rows_out) {
  const uint32_t k = kmer_length;
  const size_t nm = t.size();
  if (k < 2 || names.size() != nm || S.size() != nm * (size_t)k * HS_ALPHABET || family.size() != nm ||
      offset.size() != nm) {
    if (err) *err = k < 2 ? "kmer length 1 is not supported on a FASTA database" : "the profiles do not match the kmer length";
    return HS_ERR_INVALID;
  }
  std::vector<uint32_t> m_group;
  std::vector<std::string> fam_names;
  if (!FamilyGroups(family, &m_group, &fam_names, err)) return HS_ERR_INVALID;
  const size_t n_seq = db.start.empty() ? 0 : db.start.size() - 1;
  hs_handle* h = nullptr;
  uint64_t n_win = 0;
  std::vector<uint32_t> win_pos;
  std::vector<uint64_t> id_start;
  hs_status st = (hs_status)OpenWindowsIndex(db, k, device, &h, &n_win, &win_pos, &id_start, err);
  HandleCloser closer = {h};
  if (st != HS_OK) return st;
  if (n_windows) *n_windows = n_win;
  const std::vector<double> t_group(fam_names.size(), threshold ? *threshold : 0.0);
  std::vector<uint32_t> rg, rs, rc, rbm, rid, rlo, rhi;
  std::vector<int32_t> rd;
  std::vector<double> rsum, rsc;
  uint64_t n_rows = 0, n_hits = 0;
  for (uint64_t cap = 0;;) {  // the row count, then the rows
    for (std::vector<uint32_t>* v : {&rg, &rs, &rc, &rbm, &rid, &rlo, &rhi}) v->resize(cap);
    rd.resize(cap), rsum.resize(cap), rsc.resize(cap);
    st = hs_pssm_family_scan(h, S.data(), t.data(), nm, m_group.data(), fam_names.size(), offset.data(), id_start.data(),
                             n_seq, min_blocks, threshold ? t_group.data() : nullptr, rg.data(), rs.data(), rd.data(),
                             rc.data(), rsum.data(), rsc.data(), rbm.data(), rid.data(), rlo.data(), rhi.data(), cap,
                             &n_rows, &n_hits, nullptr, nullptr);
    if (st == HS_ERR_CAPACITY && n_rows > cap) {
      cap = n_rows;
      continue;
    }
    break;
  }
  if (st != HS_OK) {
    if (err) *err = std::string("hs_pssm_family_scan: ") + hs_last_error(h);
    return st;
  }
  if (n_hits_out) *n_hits_out = n_hits;
  if (n_rows_out) *n_rows_out = n_rows;
  std::ofstream fout(output_file.c_str());
  char sum[64], num[64];
  for (uint64_t i = 0; i < n_rows; ++i) {  // offsets are residue offsets in the protein, as the scan's window names
    const size_t s = rs[i];
    const uint64_t at = db.start[s], w0 = id_start[s];
    snprintf(sum, sizeof(sum), "%.17g", rsum[i]);
    snprintf(num, sizeof(num), "%.17g", rsc[i]);
    fout << fam_names[rg[i]] << " " << ProteinLabel(db, s) << " " << rd[i] << " " << rc[i] << " " << sum << " "
         << names[rbm[i]] << " " << (win_pos[rid[i]] - at) << " " << num << " " << (win_pos[w0 + rlo[i]] - at) << " "
         << (win_pos[w0 + rhi[i]] - at) << "\n";
  }
  fout.close();
  return HS_OK;
}

int FamilyChain(const ProteinDB& db, uint32_t kmer_length, const std::vector<std::string>& names,
                const std::vector<double>& S, const std::vector<double>& t, const std::vector<std::string>& family,
                const std::vector<uint32_t>& offset, uint32_t max_shift, double gap_open, double gap_ext,
                uint32_t min_blocks, const double* threshold, const std::string& output_file, int device,
                std::string* err, uint64_t* n_windows, uint64_t* n_hits_out, uint64_t* n_rows_out) {
  const uint32_t k = kmer_length;
  const size_t nm = t.size();
  if (k < 2 || names.size() != nm || S.size() != nm * (size_t)k * HS_ALPHABET || family.size() != nm ||
      offset.size() != nm) {
    if (err) *err = k < 2 ? "kmer length 1 is not supported on a FASTA database" : "the profiles do not match the kmer length";
    return HS_ERR_INVALID;
  }
  std::vector<uint32_t> m_group;
  std::vector<std::string> fam_names;
  if (!FamilyGroups(family, &m_group, &fam_names, err)) return HS_ERR_INVALID;
  for (size_t m = 1; m < nm; ++m)
    if (m_group[m] == m_group[m - 1] && offset[m] < offset[m - 1]) {
      if (err) *err = "the offsets of family " + family[m] + " decrease: a chain takes a family's profiles in block order";
      return HS_ERR_INVALID;
    }
  const size_t n_seq = db.start.empty() ? 0 : db.start.size() - 1;
  hs_handle* h = nullptr;
  uint64_t n_win = 0;
  std::vector<uint32_t> win_pos;
  std::vector<uint64_t> id_start;
  hs_status st = (hs_status)OpenWindowsIndex(db, k, device, &h, &n_win, &win_pos, &id_start, err);
  HandleCloser closer = {h};
  if (st != HS_OK) return st;
  if (n_windows) *n_windows = n_win;
  const std::vector<double> t_group(fam_names.size(), threshold ? *threshold : 0.0);
  std::vector<uint32_t> rg, rs, rc, rgap, rfm, rfi, rlm, rli;
  std::vector<int32_t> rshift;
  std::vector<double> rsc;
  uint64_t n_rows = 0, n_hits = 0;
  for (uint64_t cap = 0;;) {  // the row count, then the rows
    for (std::vector<uint32_t>* v : {&rg, &rs, &rc, &rgap, &rfm, &rfi, &rlm, &rli}) v->resize(cap);
    rshift.resize(cap), rsc.resize(cap);
    st = hs_pssm_family_chain(h, S.data(), t.data(), nm, m_group.data(), fam_names.size(), offset.data(), id_start.data(),
                              n_seq, max_shift, gap_open, gap_ext, min_blocks, threshold ? t_group.data() : nullptr,
                              rg.data(), rs.data(), rc.data(), rgap.data(), rsc.data(), rfm.data(), rfi.data(),
                              rlm.data(), rli.data(), rshift.data(), cap, &n_rows, &n_hits, nullptr, nullptr);
    if (st == HS_ERR_CAPACITY && n_rows > cap) {
      cap = n_rows;
      continue;
    }
    break;
  }
  if (st != HS_OK) {
    if (err) *err = std::string("hs_pssm_family_chain: ") + hs_last_error(h);
    return st;
  }
  if (n_hits_out) *n_hits_out = n_hits;
  if (n_rows_out) *n_rows_out = n_rows;
  std::ofstream fout(output_file.c_str());
  char num[64];
  for (uint64_t i = 0; i < n_rows; ++i) {  // offsets are residue offsets in the protein, as the scan's window names
    const size_t s = rs[i];
    const uint64_t at = db.start[s];
    snprintf(num, sizeof(num), "%.17g", rsc[i]);
    fout << fam_names[rg[i]] << " " << ProteinLabel(db, s) << " " << rc[i] << " " << rgap[i] << " " << num << " "
         << names[rfm[i]] << " " << (win_pos[rfi[i]] - at) << " " << names[rlm[i]] << " " << (win_pos[rli[i]] - at) << " "
         << rshift[i] << "\n";
  }
  fout.close();
  return HS_OK;
}

int ScanProfiles(const ProteinDB& db, uint32_t kmer_length, const std::vector<std::string>& names,
                 const std::vector<double>& S, const std::vector<double>& t, const std::string& output_file,
                 int device, std::string* err, uint64_t* n_windows, uint64_t* n_hits_out) {
  return ScanProfilesAny(db, kmer_length, names, S, t, 0, output_file, device, err, n_windows, n_hits_out);
}

int ScanProfilesTopN(const ProteinDB& db, uint32_t kmer_length, const std::vector<std::string>& names,
                     const std::vector<double>& S, const std::vector<double>& t_floor, uint32_t topn,
                     const std::string& output_file, int device, std::string* err, uint64_t* n_windows,
                     uint64_t* n_lines) {
  if (topn < 1 || topn > HS_TOPK_MAX) {
    if (err) *err = "top N must be 1 .. 64";
    return HS_ERR_INVALID;
  }
  return ScanProfilesAny(db, kmer_length, names, S, t_floor, topn, output_file, device, err, n_windows, n_lines);
}

int ScanProfilesPerSequence(const ProteinDB& db, uint32_t kmer_length, const std::vector<std::string>& names,
                            const std::vector<double>& S, const std::vector<double>& t, const std::string& output_file,
                            int device, std::string* err, uint64_t* n_windows, uint64_t* n_hits, uint64_t* n_rows) {
  uint64_t rows = 0;
  const int st = ScanProfilesAny(db, kmer_length, names, S, t, 0, output_file, device, err, n_windows, n_hits, &rows);
  if (n_rows) *n_rows = rows;
  return st;
}

bool WritePssmFile(const std::string& path, uint32_t kmer_length, const std::vector<std::string>& names,
                   const std::vector<double>& S, const std::vector<double>& t, std::string* err) {
  const size_t nm = t.size(), row = HS_ALPHABET;
  if (names.size() != nm || S.size() != nm * (size_t)kmer_length * row) {
    if (err) *err = "the profiles do not match the kmer length";
    return false;
  }
  std::ofstream fout(path.c_str());
  char num[64];
  for (size_t m = 0; m < nm && fout; ++m) {
    snprintf(num, sizeof(num), "%.17g", t[m]);
    fout << ">" << names[m] << " " << num << "\n";
    for (size_t p = 0; p < kmer_length; ++p)
      for (size_t a = 0; a < row; ++a) {
        snprintf(num, sizeof(num), "%.17g", S[(m * kmer_length + p) * row + a]);
        fout << num << (a + 1 < row ? " " : "\n");
      }
  }
  fout.close();
  if (!fout) {
    if (err) *err = "cannot write " + path;
    return false;
  }
  return true;
}

// The refine loop over the database's windows under either threshold rule (t or rank, exactly one) and either count
// (neff_rule < 0: every site counts 1 -- hs_pssm_refine / hs_pssm_refine_rank; 0 or 1: hs_pssm_refine_weighted).
static int RefineAny(const ProteinDB& db, uint32_t kmer_length, const std::vector<double>& S, const std::vector<double>* t,
                     const std::vector<uint64_t>* rank, int neff_rule, uint32_t n_iter, bool one_per_protein,
                     double pseudo, int device, std::vector<double>* S_out, std::vector<double>* t_out, uint32_t* iters,
                     bool* converged, std::string* err) {
  const uint32_t k = kmer_length;
  const size_t nm = rank ? rank->size() : t->size();
  if (k < 2 || S.size() != nm * (size_t)k * HS_ALPHABET) {
    if (err) *err = k < 2 ? "kmer length 1 is not supported on a FASTA database" : "the profiles do not match the kmer length";
    return HS_ERR_INVALID;
  }
  const size_t n_seq = db.start.empty() ? 0 : db.start.size() - 1;
  hs_handle* h = nullptr;
  uint64_t n_win = 0;
  std::vector<uint32_t> win_pos;
  std::vector<uint64_t> id_start;
  hs_status st = (hs_status)OpenWindowsIndex(db, k, device, &h, &n_win, &win_pos, &id_start, err);
  HandleCloser closer = {h};
  if (st != HS_OK) return st;
  S_out->assign(S.size(), 0.0);
  if (rank) t_out->assign(nm, 0.0);
  const uint64_t* const ids = one_per_protein ? id_start.data() : nullptr;
  uint32_t done = 0, conv = 0;
  const char* name = neff_rule >= 0 ? "hs_pssm_refine_weighted" : rank ? "hs_pssm_refine_rank" : "hs_pssm_refine";
  if (neff_rule >= 0)
    st = hs_pssm_refine_weighted(h, S.data(), rank ? nullptr : t->data(), rank ? rank->data() : nullptr, nm, ids, n_seq,
                                 nullptr, pseudo, (uint32_t)neff_rule, n_iter, S_out->data(),
                                 rank ? t_out->data() : nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &done, &conv);
  else if (rank)
    st = hs_pssm_refine_rank(h, S.data(), rank->data(), nm, ids, n_seq, nullptr, pseudo, n_iter, S_out->data(),
                             t_out->data(), nullptr, nullptr, &done, &conv);
  else
    st = hs_pssm_refine(h, S.data(), t->data(), nm, ids, n_seq, nullptr, pseudo, n_iter, S_out->data(), nullptr, nullptr,
                        &done, &conv);
  if (st != HS_OK) {
    if (err) *err = std::string(name) + ": " + hs_last_error(h);
    return st;
  }
  if (iters) *iters = done;
  if (converged) *converged = conv != 0;
  return HS_OK;
}

int RefineProfiles(const ProteinDB& db, uint32_t kmer_length, const std::vector<double>& S, const std::vector<double>& t,
                   uint32_t n_iter, bool one_per_protein, double pseudo, int device, std::vector<double>* S_out,
                   uint32_t* iters, bool* converged, std::string* err) {
  return RefineAny(db, kmer_length, S, &t, nullptr, -1, n_iter, one_per_protein, pseudo, device, S_out, nullptr, iters,
                   converged, err);
}

int RefineProfilesWeighted(const ProteinDB& db, uint32_t kmer_length, const std::vector<double>& S,
                           const std::vector<double>* t, const std::vector<uint64_t>* rank, bool neff_columns,
                           uint32_t n_iter, bool one_per_protein, double pseudo, int device, std::vector<double>* S_out,
                           std::vector<double>* t_out, uint32_t* iters, bool* converged, std::string* err) {
  if ((t != nullptr) == (rank != nullptr) || (rank && !t_out)) {
    if (err) *err = "exactly one of the thresholds and the ranks must be given, and t_out with the ranks";
    return HS_ERR_INVALID;
  }
  return RefineAny(db, kmer_length, S, t, rank, neff_columns ? 1 : 0, n_iter, one_per_protein, pseudo, device, S_out, t_out,
                   iters, converged, err);
}

int RankThresholds(const ProteinDB& db, uint32_t kmer_length, const std::vector<double>& S,
                   const std::vector<uint64_t>& rank, int device, std::vector<double>* t_out,
                   std::vector<uint64_t>* cnt_ge, uint64_t* n_windows, std::string* err) {
  const uint32_t k = kmer_length;
  const size_t nm = rank.size();
  if (k < 2 || S.size() != nm * (size_t)k * HS_ALPHABET) {
    if (err) *err = k < 2 ? "kmer length 1 is not supported on a FASTA database" : "the profiles do not match the kmer length";
    return HS_ERR_INVALID;
  }
  hs_handle* h = nullptr;
  uint64_t n_win = 0;
  std::vector<uint32_t> win_pos;
  std::vector<uint64_t> id_start;
  hs_status st = (hs_status)OpenWindowsIndex(db, k, device, &h, &n_win, &win_pos, &id_start, err);
  HandleCloser closer = {h};
  if (st != HS_OK) return st;
  if (n_windows) *n_windows = n_win;
  std::vector<uint64_t> ge(nm), gt(nm);
  t_out->assign(nm, 0.0);
  st = hs_pssm_rank(h, S.data(), rank.data(), nm, t_out->data(), ge.data(), gt.data(), nullptr, nullptr);
  if (st != HS_OK) {
    if (err) *err = std::string("hs_pssm_rank: ") + hs_last_error(h);
    return st;
  }
  if (cnt_ge) cnt_ge->swap(ge);
  return HS_OK;
}

int RefineProfiles(const ProteinDB& db, uint32_t kmer_length, const std::vector<double>& S,
                   const std::vector<uint64_t>& rank, uint32_t n_iter, bool one_per_protein, double pseudo, int device,
                   std::vector<double>* S_out, std::vector<double>* t_out, uint32_t* iters, bool* converged,
                   std::string* err) {
  return RefineAny(db, kmer_length, S, nullptr, &rank, -1, n_iter, one_per_protein, pseudo, device, S_out, t_out, iters,
                   converged, err);
}

// "<first token of the protein's name>#<its number>": how the search's k-mer names begin
static std::string ProteinLabel(const ProteinDB& db, size_t s) {
  std::string token;
  if (s < db.name.size()) {
    std::istringstream iss(db.name[s]);
    iss >> token;
  }
  return token + "#" + std::to_string(s);
}

int SearchProteinsPerSequence(const ProteinDB& db_first, uint32_t kmer_length, const std::vector<Point>& centers,
                              const std::vector<std::string>& center_names, const std::vector<uint8_t>* center_codes,
                              const ProteinDB* query, const uint32_t& hash_K, const uint32_t& hash_L,
                              const double& hash_W, const double& hash_R, const std::string& output_file,
                              const Planes& planes, int device, std::string* err, std::vector<uint64_t>* table_sizes,
                              uint64_t* n_windows, uint32_t probes, const std::vector<double>* radii,
                              const std::vector<ProteinDB>* more) {
  const uint32_t dim = 8 * kmer_length, k = kmer_length;
  const bool appended = more && !more->empty();
  std::vector<uint64_t> part_end;
  const ProteinDB joined = appended ? JoinProteinDBs(db_first, *more, &part_end) : ProteinDB();
  const ProteinDB& db = appended ? joined : db_first;
  const size_t n_groups = query ? (query->start.empty() ? 0 : query->start.size() - 1) : centers.size();
  if (!RadiiMatch(radii, n_groups, err)) return HS_ERR_INVALID;
  if (!query && center_codes && center_codes->size() != centers.size() * (size_t)k) {
    if (err) *err = "centre codes do not match the centres";
    return HS_ERR_INVALID;
  }
  if (k < 2 || planes.dim != dim || planes.K != hash_K || planes.L != hash_L || planes.W != hash_W) {
    if (err) *err = k < 2 ? "kmer length 1 is not supported on a FASTA database" : "planes do not match (dim, K, L, W)";
    return HS_ERR_INVALID;
  }
  // sequences cut at unknown letters, as in SearchProteinsSharded: windows never cross a cut
  std::vector<uint8_t> res(db.residues);
  std::vector<uint64_t> seg;
  const size_t n_seq = db.start.empty() ? 0 : db.start.size() - 1;
  for (size_t s = 0; s < n_seq; ++s) {
    seg.push_back(db.start[s]);
    for (uint64_t p = db.start[s]; p < db.start[s + 1]; ++p)
      if (res[p] == ProteinDB::kUnknown) {
        res[p] = 0;
        seg.push_back(p);
        seg.push_back(p + 1);
      }
  }
  seg.push_back(db.residues.size());
  // the queries: the centres, every one its own group; or every window (free of unknown letters) of every query
  // protein, grouped by protein, with its offset in the protein
  std::vector<double> flat;
  std::vector<uint8_t> qcodes;
  std::vector<uint32_t> q_group, q_off;
  std::vector<double> q_radii;
  uint64_t nq = centers.size();
  if (query) {
    for (size_t g = 0; g < n_groups; ++g) {
      const uint64_t a = query->start[g], b = query->start[g + 1];
      uint64_t known = 0;  // residues since the last unknown letter
      for (uint64_t p = a; p < b; ++p) {
        known = query->residues[p] == ProteinDB::kUnknown ? 0 : known + 1;
        if (known < k) continue;
        qcodes.insert(qcodes.end(), query->residues.begin() + (p + 1 - k), query->residues.begin() + (p + 1));
        q_group.push_back((uint32_t)g);
        q_off.push_back((uint32_t)(p + 1 - k - a));
        if (radii) q_radii.push_back((*radii)[g]);
      }
    }
    nq = q_group.size();
  } else if (center_codes) {
    qcodes = *center_codes;
  } else if (!FlattenCenters(centers, dim, &flat, err)) {
    return HS_ERR_INVALID;
  }
  const double* rad = !radii ? nullptr : query ? q_radii.data() : radii->data();
  static const double no_radius = 0.0;
  if (radii && !nq) rad = &no_radius;
  hs_params prm;
  memset(&prm, 0, sizeof(prm));
  prm.k = k;
  prm.K = hash_K;
  prm.L = hash_L;
  prm.W = hash_W;
  prm.alphabet = HS_ALPHABET;
  prm.device = device;
  hs_handle* h = nullptr;
  hs_status st = hs_create(&prm, planes.a.data(), planes.b.data(), &HS_AA_COORDS[0][0], &h);
  if (st != HS_OK) {
    if (err) *err = std::string("hs_create: ") + (h ? hs_last_error(h) : "no usable gfx950 device");
    hs_destroy(h);
    return st;
  }
  HandleCloser closer = {h};
  if (probes && (st = hs_set_multiprobe(h, probes)) != HS_OK) {
    if (err) *err = std::string("hs_set_multiprobe: ") + hs_last_error(h);
    return st;
  }
  uint64_t n_win = 0;
  std::vector<uint32_t> win_pos(res.size() + 1);
  st = BuildWindowsInParts(h, res, seg, part_end, &n_win, win_pos.data());
  if (st != HS_OK) {
    if (err) *err = std::string("index build: ") + hs_last_error(h);
    return st;
  }
  if (n_windows) *n_windows = n_win;
  hs_index_info info;
  if (table_sizes && hs_index_info_get(h, &info) == HS_OK) table_sizes->assign(info.n_buckets, info.n_buckets + prm.L);
  // protein s owns the windows that start inside it: their ids are consecutive (windows are numbered by position)
  std::vector<uint64_t> id_start(n_seq + 1);
  for (size_t s = 0; s <= n_seq; ++s)
    id_start[s] = (uint64_t)(std::lower_bound(win_pos.begin(), win_pos.begin() + n_win, db.start.empty() ? 0 : db.start[s]) -
                             win_pos.begin());
  id_start[n_seq] = n_win;
  std::vector<uint32_t> o_group, o_seq, o_count, o_q, o_id, o_lo, o_hi;
  std::vector<int32_t> o_diag;
  std::vector<double> o_dist;
  uint64_t n_rows = 0, n_hits = 0;
  for (uint64_t cap = 0;;) {  // the row count, then the rows
    for (std::vector<uint32_t>* v : {&o_group, &o_seq, &o_count, &o_q, &o_id, &o_lo, &o_hi}) v->resize(cap);
    o_diag.resize(cap);
    o_dist.resize(cap);
    st = hs_seq_match(h, qcodes.empty() ? flat.data() : nullptr, qcodes.empty() ? nullptr : qcodes.data(), nq, hash_R,
                      rad, query ? q_group.data() : nullptr, query ? n_groups : nq, query ? q_off.data() : nullptr,
                      id_start.data(), n_seq, o_group.data(), o_seq.data(), o_diag.data(), o_count.data(),
                      o_dist.data(), o_q.data(), o_id.data(), o_lo.data(), o_hi.data(), cap, &n_rows, &n_hits);
    if (st == HS_ERR_CAPACITY && n_rows > cap) {
      cap = n_rows;
      continue;
    }
    break;
  }
  if (st != HS_OK) {
    if (err) *err = std::string("hs_seq_match: ") + hs_last_error(h);
    return st;
  }
  // one line per row: the group (centre, or query protein), the protein, the count, the residue offset of the best
  // window, its distance (%.17g reads back to the same double), the first and the last matched offset; with query
  // proteins the diagonal last
  std::ofstream fout(output_file.c_str());
  for (uint64_t i = 0; i < n_rows; ++i) {
    const size_t s = o_seq[i];
    const uint64_t base = db.start[s];
    char num[40];
    snprintf(num, sizeof(num), "%.17g", o_dist[i]);
    fout << (query ? ProteinLabel(*query, o_group[i]) : center_names[o_group[i]]) << " " << ProteinLabel(db, s) << " "
         << o_count[i] << " " << (win_pos[o_id[i]] - base) << " " << num << " "
         << (win_pos[id_start[s] + o_lo[i]] - base) << " " << (win_pos[id_start[s] + o_hi[i]] - base);
    if (query) fout << " " << o_diag[i];
    fout << std::endl;
  }
  fout.close();
  return HS_OK;
}

int64_t Protein2Datapoints(const ProteinDB& db, uint32_t kmer_length, uint32_t num_of_protein_out,
                           const std::string& output_file, uint32_t seed) {
  std::ofstream fout(output_file.c_str());
  if (!fout) return -1;
  const size_t n_seq = db.start.empty() ? 0 : db.start.size() - 1;
  const char* letters = HS_CODE_TO_LETTER;
  std::unordered_set<std::string> seen;
  int64_t cnt = 0;
  srand(seed);
  for (size_t i = 0; i < n_seq; ++i) {
    if (i >= num_of_protein_out) break;  // :42
    const uint64_t len = db.start[i + 1] - db.start[i];
    if (len < kmer_length) continue;
    std::string name;
    if (i < db.name.size()) {
      std::istringstream iss(db.name[i]);  // :62-64
      iss >> name;
    }
    for (uint64_t j = 0; j + kmer_length <= len;) {
      const uint64_t pos = db.start[i] + j;
      std::string kmer(kmer_length, '?');
      bool known = true;
      for (uint32_t p = 0; p < kmer_length; ++p) {
        const uint8_t row = db.residues[pos + p];
        if (row == ProteinDB::kUnknown) known = false;
        else kmer[p] = letters[row];
      }
      if (!known || seen.find(kmer) != seen.end()) {  // :49-53
        j += 30 + rand() % 20;
        continue;
      }
      seen.insert(kmer);
      fout << name << "#" << i << "$" << j << "@" << kmer << "*" << cnt << std::endl;  // :65
      for (uint32_t p = 0; p < kmer_length; ++p)                                        // :22-28
        for (uint32_t c = 0; c < 8; ++c) {
          if (p || c) fout << " ";
          fout << HS_AA_COORDS[db.residues[pos + p]][c];
        }
      fout << std::endl;
      ++cnt;
      j += 30 + rand() % 20;  // :70-71
    }
  }
  return cnt;
}

bool ReadPclusterFasta(const std::string& path, uint32_t unknown_seed, PclusterDB* db) {
  std::ifstream fin(path.c_str());
  if (!fin) return false;
  db->names.clear();
  db->seqs.clear();
  std::mt19937 gen(unknown_seed);
  std::string line, sequence;
  bool open = false;
  while (std::getline(fin, line)) {  // read_proteins.cpp:13-35
    if (!line.empty() && line[line.size() - 1] == '\r') line.erase(line.size() - 1);
    if (!line.empty() && line[0] == '>') {
      if (!sequence.empty()) {
        db->seqs.push_back(sequence);
        sequence.clear();
      }
      const size_t sp = line.find_first_of(' ');
      db->names.push_back(sp == std::string::npos ? line.substr(1) : line.substr(1, sp - 1));
      open = true;
      continue;
    }
    for (size_t i = 0; i < line.size(); ++i) {
      const char c = line[i];
      if (c >= 'A' && c <= 'Z' && HS_LETTER_TO_CODE[c - 'A'] >= 0)
        sequence.push_back(c);
      else if (isalpha((unsigned char)c))
        sequence.push_back(HS_CODE_TO_LETTER[gen() % 20]);
    }
  }
  if (!sequence.empty()) db->seqs.push_back(sequence);
  (void)open;
  return true;
}

int PreClustering(const PclusterDB& db, int device,
                  std::map<uint64_t, std::vector<uint32_t> >* hash_buckets, std::string* err) {
  hash_buckets->clear();
  const uint32_t bits = 16;  // pcluster.cpp:13-15: feature_size = 8^HASHLEN, bit_num = 16, sigma = 0.2
  std::vector<double> w((size_t)bits * HS_KLSH_FEATURES), b(bits), t(bits);
  hs_status st = hs_klsh_draw_planes(HS_KLSH_FEATURES, bits, 0.2, w.data(), b.data(), t.data());
  if (st != HS_OK) {
    if (err) *err = "hs_klsh_draw_planes failed";
    return st;
  }
  std::vector<uint8_t> classes;
  std::vector<uint64_t> start(1, 0);
  for (size_t i = 0; i < db.seqs.size(); ++i) {
    for (size_t p = 0; p < db.seqs[i].size(); ++p)
      classes.push_back((uint8_t)HS_REDUCED_CLASS[db.seqs[i][p] - 'A']);
    start.push_back(classes.size());
  }
  std::vector<uint64_t> codes(db.seqs.size());
  char msg[256] = {0};
  st = hs_klsh_codes(device, classes.data(), classes.size(), start.data(), db.seqs.size(), w.data(),
                     b.data(), t.data(), bits, codes.data(), nullptr, msg, sizeof(msg));
  if (st != HS_OK) {
    if (err) *err = std::string("hs_klsh_codes: ") + msg;
    return st;
  }
  for (size_t i = 0; i < codes.size(); ++i)
    if (codes[i] != HS_KLSH_NONE) (*hash_buckets)[codes[i]].push_back((uint32_t)i);  // pcluster.cpp:34
  return HS_OK;
}

bool ReadKmerFasta(const std::string& path, std::vector<Kmer>* kmers) {
  std::ifstream fin(path.c_str());
  if (!fin) return false;
  std::string tok;
  while (fin >> tok) {
    if (tok[0] == '>') {
      Kmer km;
      km.name = tok.substr(1);
      fin >> km.seq;
      kmers->push_back(km);
    }
  }
  return true;
}

bool ReadPlanesFile(const std::string& path, uint32_t dim, uint32_t K, uint32_t L, double W, Planes* planes,
                    std::string* err) {
  std::ifstream fin(path.c_str(), std::ios::binary);
  if (!fin) {
    if (err) *err = "cannot open " + path;
    return false;
  }
  planes->dim = dim;
  planes->K = K;
  planes->L = L;
  planes->W = W;
  planes->a.assign((size_t)L * K * dim, 0.0);
  planes->b.assign((size_t)L * K, 0.0);
  fin.read(reinterpret_cast<char*>(planes->a.data()), planes->a.size() * sizeof(double));
  fin.read(reinterpret_cast<char*>(planes->b.data()), planes->b.size() * sizeof(double));
  char extra;
  if (!fin || fin.read(&extra, 1)) {
    if (err) *err = path + " does not hold L*K*dim + L*K doubles for these -l/-K/-L";
    return false;
  }
  for (double v : planes->a)
    if (!std::isfinite(v)) {
      if (err) *err = path + " holds a non-finite plane coefficient";
      return false;
    }
  return true;
}

bool CentersFromKmers(const std::vector<Kmer>& kmers, uint32_t kmer_length, std::vector<std::string>* names,
                      std::vector<Point>* centers, std::string* err, std::vector<uint8_t>* codes) {
  for (const Kmer& km : kmers) {
    if (km.seq.size() != kmer_length) {
      if (err) *err = "centre " + km.name + " does not have " + std::to_string(kmer_length) + " residues";
      return false;
    }
    Point pt;
    pt.data.resize(8 * (size_t)kmer_length);
    for (uint32_t p = 0; p < kmer_length; ++p) {
      const char c = km.seq[p];
      const int row = (c >= 'A' && c <= 'Z') ? HS_LETTER_TO_CODE[c - 'A'] : -1;  // base[], util.hpp:92
      if (row < 0) {
        if (err) *err = "centre " + km.name + " has a letter outside the 20-letter alphabet";
        return false;
      }
      for (int j = 0; j < 8; ++j) pt.data[8 * p + j] = HS_AA_COORDS[row][j];  // hclust2.cpp:57-59
      if (codes) codes->push_back((uint8_t)row);
    }
    names->push_back(km.name);
    centers->push_back(pt);
  }
  return true;
}

namespace {

// The residue codes of hclust2's k-mers (KmerToCoordinates, hclust2.cpp:49-62), after the check that the planes
// are the ones the options name: 0, or HS_ERR_INVALID with *err set.
int ClusterCodes(const std::vector<Kmer>& kmers, uint32_t hash_K, uint32_t hash_L, double hash_W, const Planes& planes,
                 uint32_t unknown_seed, std::vector<uint8_t>* codes, std::string* err) {
  const uint32_t dim = planes.dim, k = dim / 8;
  if (dim == 0 || dim % 8 != 0 || planes.K != hash_K || planes.L != hash_L || planes.W != hash_W) {
    if (err) *err = "planes do not match (dim, K, L, W)";
    return HS_ERR_INVALID;
  }
  const size_t n = kmers.size();
  codes->resize(n * (size_t)k);
  std::minstd_rand unknown(unknown_seed);
  for (size_t i = 0; i < n; ++i) {
    if (kmers[i].seq.size() != k) {
      if (err) *err = "k-mer '" + kmers[i].name + "' does not have length " + std::to_string(k);
      return HS_ERR_INVALID;
    }
    for (uint32_t p = 0; p < k; ++p) {
      const int c = kmers[i].seq[p] - 'A';
      int code = (c >= 0 && c < 26) ? HS_LETTER_TO_CODE[c] : -1;  // base[], util.hpp:92
      if (code < 0) code = (int)(unknown() % 20);
      (*codes)[i * k + p] = (uint8_t)code;
    }
  }
  return HS_OK;
}

}  // namespace

int ClusterCenters(hs_handle* h, const std::vector<Kmer>& kmers, const std::vector<uint32_t>& label, uint32_t min_size,
                   const std::string& output_file, std::string* err, uint64_t* n_centers) {
  hs_params prm;
  if (!h || hs_get_params(h, &prm) != HS_OK || label.size() != kmers.size()) {
    if (err) *err = "ClusterCenters: no handle, or not one label per k-mer";
    return HS_ERR_INVALID;
  }
  const uint32_t dim = 8 * prm.k;
  // one call: n / min_size rows hold every result (include/hsearch.h)
  if (!min_size) {
    if (err) *err = "ClusterCenters: min_size must be at least 1";
    return HS_ERR_INVALID;
  }
  const uint64_t room = label.size() / min_size;
  uint64_t rows = 0;
  std::vector<uint32_t> row_label(room), row_size(room);
  std::vector<double> centroid(room * dim);
  const hs_status pst = hs_cluster_profile(h, label.data(), min_size, row_label.data(), row_size.data(), nullptr,
                                           centroid.data(), room, &rows);
  if (pst != HS_OK) {
    if (err) *err = std::string("hs_cluster_profile: ") + hs_last_error(h);
    return pst;
  }
  std::vector<uint32_t> medoid(rows);
  std::vector<double> max_d2(rows), radius(rows);
  std::vector<MotifFamily> families(rows);
  std::vector<Point> centers(rows);
  for (uint64_t r = 0; r < rows; ++r) {
    families[r].name = kmers[row_label[r]].name + ":size" + std::to_string(row_size[r]);
    centers[r].data.assign(centroid.begin() + r * dim, centroid.begin() + (r + 1) * dim);
  }
  if (!Cluster2DataPoint(families, centers, output_file)) {
    if (err) *err = "cannot write " + output_file + "hclust.format.txt";
    return HS_ERR_IO;
  }
  // the centroids as the points file holds them (6 significant digits): what a search is given as its centres
  std::vector<std::string> names;
  std::vector<Point> written;
  if (!ReadPointsFile(output_file + "hclust.format.txt", dim, &names, &written) || written.size() != rows) {
    if (err) *err = "cannot read " + output_file + "hclust.format.txt back";
    return HS_ERR_IO;
  }
  std::vector<double> flat(rows * dim);
  for (uint64_t r = 0; r < rows; ++r) std::copy(written[r].data.begin(), written[r].data.end(), flat.begin() + r * dim);
  const hs_status st = hs_cluster_radii(h, label.data(), min_size, flat.data(), rows, max_d2.data(), radius.data(), medoid.data());
  if (st != HS_OK) {
    if (err) *err = std::string("hs_cluster_radii: ") + hs_last_error(h);
    return st;
  }
  std::ofstream fout((output_file + "hclust.radii.txt").c_str());
  if (!fout) {
    if (err) *err = "cannot write " + output_file + "hclust.radii.txt";
    return HS_ERR_IO;
  }
  for (uint64_t r = 0; r < rows; ++r) {
    char num[64];
    snprintf(num, sizeof(num), "%.17g", radius[r]);
    fout << families[r].name << " " << num << std::endl;
  }
  if (n_centers) *n_centers = rows;
  return HS_OK;
}

int ClusterProfiles(hs_handle* h, const std::vector<Kmer>& kmers, const std::vector<uint32_t>& label,
                    const ClusterProfileOptions& opt, const std::string& output_file, std::string* err,
                    uint64_t* n_profiles) {
  hs_params prm;
  if (!h || hs_get_params(h, &prm) != HS_OK || label.size() != kmers.size()) {
    if (err) *err = "ClusterProfiles: no handle, or not one label per k-mer";
    return HS_ERR_INVALID;
  }
  const bool pseudo_ok = opt.pseudo > 0.0 && opt.pseudo <= 1.7976931348623157e308;
  if (!opt.min_size || opt.weights < 0 || opt.weights > 2 || opt.threshold < 0 || opt.threshold > 1 || !pseudo_ok) {
    if (err) *err = "ClusterProfiles: min_size must be at least 1, weights 0 .. 2, threshold 0 or 1, pseudo finite and > 0";
    return HS_ERR_INVALID;
  }
  const uint32_t k = prm.k, A = HS_ALPHABET;
  const size_t cells = (size_t)k * A, n = label.size();
  const uint64_t room = n / opt.min_size;
  uint64_t rows = 0;
  std::vector<uint32_t> row_label(room), row_size(room), counts(room * cells), distinct(room);
  std::vector<uint64_t> wcounts, wsum;
  hs_status st;
  const char* what = "hs_cluster_weighted_profile";
  if (opt.weights) {
    wcounts.resize(room * cells);
    wsum.resize(room);
    st = hs_cluster_weighted_profile(h, label.data(), opt.min_size, row_label.data(), row_size.data(), counts.data(),
                                     wcounts.data(), wsum.data(), distinct.data(), room, &rows);
  } else {
    what = "hs_cluster_profile";
    std::vector<double> centroid(room * 8 * k);
    st = hs_cluster_profile(h, label.data(), opt.min_size, row_label.data(), row_size.data(), counts.data(),
                            centroid.data(), room, &rows);
  }
  std::vector<double> S(rows * cells), t(rows);
  double bg[HS_ALPHABET];
  if (st == HS_OK && rows) {
    // the background: the residue composition of all n input k-mers -- the counts of one cluster that holds them all
    what = "hs_cluster_profile (composition)";
    const std::vector<uint32_t> everything(n, 0u);
    std::vector<uint32_t> all_counts(cells), one(2);
    std::vector<double> centroid(8 * k);
    uint64_t one_row = 0;
    st = hs_cluster_profile(h, everything.data(), 1, &one[0], &one[1], all_counts.data(), centroid.data(), 1, &one_row);
    if (st == HS_OK && hs_pssm_background(all_counts.data(), k, A, bg) != HS_OK) {
      if (err) *err = "ClusterProfiles: no background";
      return HS_ERR_INVALID;
    }
  }
  if (st == HS_OK && rows) {
    if (opt.weights) {
      std::vector<double> n_eff(rows);
      for (uint64_t r = 0; r < rows; ++r)
        n_eff[r] = opt.weights == 1 ? (double)row_size[r] : (double)distinct[r] / (double)k;
      if (hs_pssm_log_odds_weighted(wcounts.data(), wsum.data(), n_eff.data(), rows, k, A, bg, opt.pseudo, S.data()) != HS_OK) {
        if (err) *err = "hs_pssm_log_odds_weighted refused the weighted counts";
        return HS_ERR_INVALID;
      }
    } else if (hs_pssm_log_odds(counts.data(), rows, k, A, bg, opt.pseudo, S.data()) != HS_OK) {
      if (err) *err = "hs_pssm_log_odds refused the counts";
      return HS_ERR_INVALID;
    }
    if (opt.threshold == 0) {
      what = "hs_cluster_pssm_cover";
      std::vector<uint32_t> argmin(rows);
      st = hs_cluster_pssm_cover(h, label.data(), opt.min_size, S.data(), rows, t.data(), argmin.data());
    } else {
      what = "hs_pssm_rank";
      std::vector<uint64_t> rank(rows), ge(rows), gt(rows);
      for (uint64_t r = 0; r < rows; ++r) rank[r] = row_size[r];
      st = hs_pssm_rank(h, S.data(), rank.data(), rows, t.data(), ge.data(), gt.data(), nullptr, nullptr);
    }
  }
  if (st != HS_OK) {
    if (err) *err = std::string(what) + ": " + hs_last_error(h);
    return st;
  }
  std::vector<std::string> names(rows);
  for (uint64_t r = 0; r < rows; ++r) names[r] = kmers[row_label[r]].name + ":size" + std::to_string(row_size[r]);
  std::string werr;
  if (!WritePssmFile(output_file + "hclust.pssm.txt", k, names, S, t, &werr)) {
    if (err) *err = werr;
    return HS_ERR_IO;
  }
  if (n_profiles) *n_profiles = rows;
  return HS_OK;
}

// what the clustering functions write beside the clusters file: the centres, the profiles
static int ClusterExtras(hs_handle* h, const std::vector<Kmer>& kmers, const std::vector<uint32_t>& label,
                         uint32_t centers_min_size, const ClusterProfileOptions* profiles,
                         const std::string& output_file, std::string* err) {
  if (centers_min_size) {
    const int cc = ClusterCenters(h, kmers, label, centers_min_size, output_file, err);
    if (cc != HS_OK) return cc;
  }
  if (profiles && profiles->min_size) return ClusterProfiles(h, kmers, label, *profiles, output_file, err);
  return HS_OK;
}

// Components and SingleLinkageTree: the same clusters file; tree: the labels come from hs_msf, whose tree edges go to
// <output_file>hclust.tree.txt
static int ComponentsOrTree(const std::vector<Kmer>& kmers, const uint32_t& hash_K, const uint32_t& hash_L,
                            const double& hash_W, const double& hash_R, const std::string& output_file,
                            const Planes& planes, int device, std::string* err, uint64_t* n_clusters,
                            uint32_t unknown_seed, uint32_t centers_min_size, bool tree, uint64_t* n_tree_edges,
                            const ClusterProfileOptions* profiles) {
  std::vector<uint8_t> codes;
  const int cs = ClusterCodes(kmers, hash_K, hash_L, hash_W, planes, unknown_seed, &codes, err);
  if (cs != HS_OK) return cs;
  const size_t n = kmers.size();
  hs_params prm;
  memset(&prm, 0, sizeof(prm));
  prm.k = planes.dim / 8;
  prm.K = hash_K;
  prm.L = hash_L;
  prm.W = hash_W;
  prm.device = device;
  hs_handle* h = nullptr;
  hs_status st = hs_create(&prm, planes.a.data(), planes.b.data(), nullptr, &h);
  std::vector<uint32_t> label(n);
  uint64_t n_comp = 0;
  const char* what = "hs_create";
  if (st == HS_OK) {
    what = "hs_index_build";
    st = hs_index_build(h, codes.data(), n);
  }
  std::vector<uint32_t> tree_lo, tree_hi;
  std::vector<double> tree_dist;
  if (st == HS_OK && !tree) {
    what = "hs_components";
    st = hs_components(h, hash_R, 1, label.data(), &n_comp, nullptr);  // hclust2's test: sqrt(d2) <= R
  }
  if (st == HS_OK && tree) {
    what = "hs_msf";
    tree_lo.resize(n);  // at most n - 1 tree edges: sized once
    tree_hi.resize(n);
    tree_dist.resize(n);
    hs_msf_info info;
    st = hs_msf(h, hash_R, 1, tree_lo.data(), tree_hi.data(), tree_dist.data(), n, label.data(), &info);
    if (st == HS_OK) {
      n_comp = info.n_components;
      tree_lo.resize(info.n_tree_edges);
    }
  }
  if (st != HS_OK) {
    if (err) *err = std::string(what) + ": " + (h ? hs_last_error(h) : "no handle");
    if (h) hs_destroy(h);
    return st;
  }
  const int extras = ClusterExtras(h, kmers, label, centers_min_size, profiles, output_file, err);
  if (extras != HS_OK) {
    hs_destroy(h);
    return extras;
  }
  hs_destroy(h);
  // a cluster per root in ascending id (= ascending smallest member), members in ascending id
  std::vector<uint32_t> size(n, 0), start(n + 1, 0), slot(n);
  for (size_t i = 0; i < n; ++i) ++size[label[i]];
  for (size_t i = 0; i < n; ++i) start[i + 1] = start[i] + size[i];
  std::vector<uint32_t> fill(start.begin(), start.end() - 1);
  for (size_t i = 0; i < n; ++i) slot[fill[label[i]]++] = (uint32_t)i;
  std::ofstream fout(output_file.c_str());
  uint32_t cluster_id = 0;
  for (size_t i = 0; i < n; ++i) {
    if (label[i] != i) continue;
    fout << "#clusterid:" << cluster_id++ << ":size" << size[i] << std::endl;
    for (uint32_t t = start[i]; t < start[i + 1]; ++t) fout << kmers[slot[t]].name << std::endl;
  }
  fout.close();
  if (n_clusters) *n_clusters = cluster_id;
  if (tree) {
    // one line per tree edge in merge order; %.17g reads back to the same double
    std::ofstream ftree((output_file + "hclust.tree.txt").c_str());
    if (!ftree) {
      if (err) *err = "cannot write " + output_file + "hclust.tree.txt";
      return HS_ERR_IO;
    }
    for (size_t t = 0; t < tree_lo.size(); ++t) {
      char num[64];
      snprintf(num, sizeof(num), "%.17g", tree_dist[t]);
      ftree << kmers[tree_lo[t]].name << " " << kmers[tree_hi[t]].name << " " << num << "\n";
    }
    ftree.close();
    if (n_tree_edges) *n_tree_edges = tree_lo.size();
  }
  return HS_OK;
}

int Components(const std::vector<Kmer>& kmers, const uint32_t& hash_K, const uint32_t& hash_L, const double& hash_W,
               const double& hash_R, const std::string& output_file, const Planes& planes, int device,
               std::string* err, uint64_t* n_clusters, uint32_t unknown_seed, uint32_t centers_min_size,
               const ClusterProfileOptions* profiles) {
  return ComponentsOrTree(kmers, hash_K, hash_L, hash_W, hash_R, output_file, planes, device, err, n_clusters,
                          unknown_seed, centers_min_size, false, nullptr, profiles);
}

int SingleLinkageTree(const std::vector<Kmer>& kmers, const uint32_t& hash_K, const uint32_t& hash_L,
                      const double& hash_W, const double& hash_R, const std::string& output_file, const Planes& planes,
                      int device, std::string* err, uint64_t* n_clusters, uint64_t* n_tree_edges, uint32_t unknown_seed,
                      uint32_t centers_min_size, const ClusterProfileOptions* profiles) {
  return ComponentsOrTree(kmers, hash_K, hash_L, hash_W, hash_R, output_file, planes, device, err, n_clusters,
                          unknown_seed, centers_min_size, true, n_tree_edges, profiles);
}

// Dbscan and DensityTree: the same clusters file; density: the labels come from hs_density_tree (border k-mers are
// noise), whose core distances go to <output_file>hclust.core.txt and, with tree, whose tree edges go to
// <output_file>hclust.tree.txt
static int DbscanOrDensity(const std::vector<Kmer>& kmers, const uint32_t& hash_K, const uint32_t& hash_L,
                           const double& hash_W, const double& hash_R, const uint32_t& min_pts,
                           const std::string& output_file, const Planes& planes, int device, std::string* err,
                           uint64_t* n_clusters, uint32_t unknown_seed, uint32_t centers_min_size, bool density,
                           bool tree, uint64_t* n_tree_edges, const ClusterProfileOptions* profiles) {
  std::vector<uint8_t> codes;
  const int cs = ClusterCodes(kmers, hash_K, hash_L, hash_W, planes, unknown_seed, &codes, err);
  if (cs != HS_OK) return cs;
  const size_t n = kmers.size();
  hs_params prm;
  memset(&prm, 0, sizeof(prm));
  prm.k = planes.dim / 8;
  prm.K = hash_K;
  prm.L = hash_L;
  prm.W = hash_W;
  prm.device = device;
  hs_handle* h = nullptr;
  hs_status st = hs_create(&prm, planes.a.data(), planes.b.data(), nullptr, &h);
  std::vector<uint32_t> label(n);
  hs_dbscan_counts counts;
  memset(&counts, 0, sizeof(counts));
  const char* what = "hs_create";
  if (st == HS_OK) {
    what = "hs_index_build";
    st = hs_index_build(h, codes.data(), n);
  }
  if (st == HS_OK && !density) {
    what = "hs_dbscan";
    st = hs_dbscan(h, hash_R, 1, min_pts, label.data(), nullptr, &counts);  // hclust2's test: sqrt(d2) <= R
  }
  std::vector<uint32_t> tree_lo, tree_hi;
  std::vector<double> tree_w, core;
  if (st == HS_OK && density) {
    what = "hs_density_tree";
    tree_lo.resize(n);  // at most n - 1 tree edges: sized once
    tree_hi.resize(n);
    tree_w.resize(n);
    core.resize(n);
    hs_density_info info;
    st = hs_density_tree(h, hash_R, 1, min_pts, tree_lo.data(), tree_hi.data(), tree_w.data(), n, label.data(),
                         core.data(), &info);
    if (st == HS_OK) tree_lo.resize(info.n_tree_edges);
  }
  if (st != HS_OK) {
    if (err) *err = std::string(what) + ": " + (h ? hs_last_error(h) : "no handle");
    if (h) hs_destroy(h);
    return st;
  }
  const int extras = ClusterExtras(h, kmers, label, centers_min_size, profiles, output_file, err);
  if (extras != HS_OK) {
    hs_destroy(h);
    return extras;
  }
  hs_destroy(h);
  // a cluster per label in ascending id (a label is a core k-mer of its cluster, not always its smallest member:
  // a border k-mer may have a smaller id), members in ascending id; the noise last
  std::vector<uint32_t> size(n, 0), start(n + 1, 0), slot(n);
  uint64_t noise = 0;
  for (size_t i = 0; i < n; ++i) {
    if (label[i] == HS_NOISE)
      ++noise;
    else
      ++size[label[i]];
  }
  for (size_t i = 0; i < n; ++i) start[i + 1] = start[i] + size[i];
  std::vector<uint32_t> fill(start.begin(), start.end() - 1);
  for (size_t i = 0; i < n; ++i)
    if (label[i] != HS_NOISE) slot[fill[label[i]]++] = (uint32_t)i;
  std::ofstream fout(output_file.c_str());
  uint32_t cluster_id = 0;
  for (size_t i = 0; i < n; ++i) {
    if (!size[i]) continue;
    fout << "#clusterid:" << cluster_id++ << ":size" << size[i] << std::endl;
    for (uint32_t t = start[i]; t < start[i + 1]; ++t) fout << kmers[slot[t]].name << std::endl;
  }
  if (noise) {
    fout << "#noise:size" << noise << std::endl;
    for (size_t i = 0; i < n; ++i)
      if (label[i] == HS_NOISE) fout << kmers[i].name << std::endl;
  }
  fout.close();
  if (n_clusters) *n_clusters = cluster_id;
  if (density) {
    // one line per k-mer: its name and core distance ("inf": none); %.17g reads back to the same double
    std::ofstream fcore((output_file + "hclust.core.txt").c_str());
    if (!fcore) {
      if (err) *err = "cannot write " + output_file + "hclust.core.txt";
      return HS_ERR_IO;
    }
    for (size_t i = 0; i < n; ++i) {
      char num[64];
      if (core[i] < HUGE_VAL)
        snprintf(num, sizeof(num), "%.17g", core[i]);
      else
        snprintf(num, sizeof(num), "inf");
      fcore << kmers[i].name << " " << num << "\n";
    }
    fcore.close();
  }
  if (density && tree) {
    // the format of SingleLinkageTree: one line per tree edge in merge order, the weight the merge height
    std::ofstream ftree((output_file + "hclust.tree.txt").c_str());
    if (!ftree) {
      if (err) *err = "cannot write " + output_file + "hclust.tree.txt";
      return HS_ERR_IO;
    }
    for (size_t t = 0; t < tree_lo.size(); ++t) {
      char num[64];
      snprintf(num, sizeof(num), "%.17g", tree_w[t]);
      ftree << kmers[tree_lo[t]].name << " " << kmers[tree_hi[t]].name << " " << num << "\n";
    }
    ftree.close();
  }
  if (n_tree_edges) *n_tree_edges = tree_lo.size();
  return HS_OK;
}

int Dbscan(const std::vector<Kmer>& kmers, const uint32_t& hash_K, const uint32_t& hash_L, const double& hash_W,
           const double& hash_R, const uint32_t& min_pts, const std::string& output_file, const Planes& planes, int device,
           std::string* err, uint64_t* n_clusters, uint32_t unknown_seed, uint32_t centers_min_size,
           const ClusterProfileOptions* profiles) {
  return DbscanOrDensity(kmers, hash_K, hash_L, hash_W, hash_R, min_pts, output_file, planes, device, err, n_clusters,
                         unknown_seed, centers_min_size, false, false, nullptr, profiles);
}

int DensityTree(const std::vector<Kmer>& kmers, const uint32_t& hash_K, const uint32_t& hash_L, const double& hash_W,
                const double& hash_R, const uint32_t& min_pts, const std::string& output_file, const Planes& planes,
                int device, std::string* err, bool tree, uint64_t* n_clusters, uint64_t* n_tree_edges,
                uint32_t unknown_seed, uint32_t centers_min_size, const ClusterProfileOptions* profiles) {
  return DbscanOrDensity(kmers, hash_K, hash_L, hash_W, hash_R, min_pts, output_file, planes, device, err, n_clusters,
                         unknown_seed, centers_min_size, true, tree, n_tree_edges, profiles);
}

int KnnGraph(const std::vector<Kmer>& kmers, const uint32_t& hash_K, const uint32_t& hash_L, const double& hash_W,
             const double& hash_R, const uint32_t& topk, const std::string& output_file, const Planes& planes, int device,
             std::string* err, uint64_t* n_edges, uint32_t unknown_seed) {
  if (topk < 1 || topk > HS_TOPK_MAX) {
    if (err) *err = "KnnGraph: topk must be 1 .. 64";
    return HS_ERR_INVALID;
  }
  std::vector<uint8_t> codes;
  const int cs = ClusterCodes(kmers, hash_K, hash_L, hash_W, planes, unknown_seed, &codes, err);
  if (cs != HS_OK) return cs;
  const size_t n = kmers.size();
  hs_params prm;
  memset(&prm, 0, sizeof(prm));
  prm.k = planes.dim / 8;
  prm.K = hash_K;
  prm.L = hash_L;
  prm.W = hash_W;
  prm.device = device;
  hs_handle* h = nullptr;
  hs_status st = hs_create(&prm, planes.a.data(), planes.b.data(), nullptr, &h);
  const char* what = "hs_create";
  if (st == HS_OK) {
    what = "hs_index_build";
    st = hs_index_build(h, codes.data(), n);
  }
  std::vector<uint32_t> nn_id(n * topk), nn_count(n);
  std::vector<double> nn_dist(n * topk);
  uint64_t edges = 0;
  if (st == HS_OK) {
    what = "hs_self_knn";
    st = hs_self_knn(h, hash_R, 1, topk, nn_id.data(), nullptr, nn_dist.data(), nn_count.data(), &edges);  // sqrt(d2) <= R
  }
  if (st != HS_OK) {
    if (err) *err = std::string(what) + ": " + (h ? hs_last_error(h) : "no handle");
    if (h) hs_destroy(h);
    return st;
  }
  hs_destroy(h);
  std::ofstream fout((output_file + "hclust.knn.txt").c_str());
  if (!fout) {
    if (err) *err = "cannot write " + output_file + "hclust.knn.txt";
    return HS_ERR_IO;
  }
  for (size_t i = 0; i < n; ++i) {
    fout << kmers[i].name << " " << nn_count[i];
    for (uint32_t r = 0; r < topk && r < nn_count[i]; ++r) {
      char num[64];
      snprintf(num, sizeof(num), "%.17g", nn_dist[i * topk + r]);
      fout << " " << kmers[nn_id[i * topk + r]].name << " " << num;
    }
    fout << "\n";
  }
  fout.close();
  if (n_edges) *n_edges = edges;
  return HS_OK;
}

int Clustering(const std::vector<Kmer>& kmers, const uint32_t& hash_K, const uint32_t& hash_L,
               const double& hash_W, const double& hash_R, const std::string& output_file,
               const Planes& planes, int device, uint32_t unknown_seed, std::string* err,
               uint64_t* n_clusters) {
  std::vector<uint8_t> codes;
  const int cs = ClusterCodes(kmers, hash_K, hash_L, hash_W, planes, unknown_seed, &codes, err);
  if (cs != HS_OK) return cs;
  const size_t n = kmers.size();
  const uint32_t k = planes.dim / 8;
  hs_params prm;
  memset(&prm, 0, sizeof(prm));
  prm.k = k;
  prm.K = hash_K;
  prm.L = hash_L;
  prm.W = hash_W;
  prm.device = device;
  std::vector<uint8_t> merged(n);
  std::vector<uint32_t> owner(n), table(n);
  char msg[512] = {0};
  const hs_status st = hs_clustering(&prm, planes.a.data(), planes.b.data(), nullptr, codes.data(), n,
                                     hash_R, merged.data(), owner.data(), table.data(), msg, sizeof(msg));
  if (st != HS_OK) {
    if (err) *err = msg;
    return st;
  }
  // members of a cluster in absorption order: table by table, ascending id inside a table
  std::vector<std::vector<uint32_t> > members(n);
  std::vector<uint32_t> order;
  for (size_t i = 0; i < n; ++i)
    if (merged[i] == 2) order.push_back((uint32_t)i);
  std::stable_sort(order.begin(), order.end(),
                   [&](uint32_t x, uint32_t y) { return table[x] < table[y]; });
  for (uint32_t i : order) members[owner[i]].push_back(i);
  std::ofstream fout(output_file.c_str());
  uint32_t cluster_id = 0;
  for (size_t i = 0; i < n; ++i) {
    if (merged[i] == 1 || merged[i] == 0) {
      fout << "#clusterid:" << cluster_id++ << ":size" << members[i].size() + 1 << std::endl;
      fout << kmers[i].name << std::endl;
      for (uint32_t j : members[i]) fout << kmers[j].name << std::endl;
    }
  }
  fout.close();
  if (n_clusters) *n_clusters = cluster_id;
  return HS_OK;
}

namespace {

struct MotifRes {
  std::string motif, protein;
  double dis;
};

bool ResLess(const MotifRes& a, const MotifRes& b) {
  if (a.motif == b.motif) return a.protein < b.protein;
  return a.motif < b.motif;
}

int ResCompare(const MotifRes& a, const MotifRes& b) {
  if (a.motif == b.motif) {
    if (a.protein == b.protein) return 0;
    return a.protein > b.protein ? 1 : -1;
  }
  return a.motif > b.motif ? 1 : -1;
}

// weight(): 1 below distance 24, then 1/(dis-24) clipped to [0,1]; inconsistent ground truth
// (dis > R + 0.1) is reported through *bad instead of exit(0).
double Weight(double dis, double R, bool* bad) {
  if (dis > R + 0.1) {
    *bad = true;
    return 0;
  }
  if (dis < 0.0000001) return 1;
  if (dis < 24) return 1;
  double w = 1 / (dis - 24);
  if (w > 1) return 1;
  if (w < 0) return 1;
  return w;
}

}  // namespace

double Evaluate(const std::string& ground_truth, const std::string& output_file, const double& hash_R) {
  std::vector<MotifRes> brute, found;
  MotifRes r;
  {
    std::ifstream fin(ground_truth.c_str());
    while (fin >> r.motif >> r.protein >> r.dis) brute.push_back(r);
  }
  {
    std::ifstream fin(output_file.c_str());
    while (fin >> r.motif >> r.protein >> r.dis) found.push_back(r);
  }
  std::sort(found.begin(), found.end(), ResLess);
  size_t i = 0, j = 0;
  double tp = 0.0, fn = 0.0;
  bool bad = false;
  std::unordered_map<int, int> tp_map, fn_map;  // distance decile histogram
  while (i < brute.size() && j < found.size()) {
    const int cmp = ResCompare(brute[i], found[j]);
    if (cmp == 0) {
      tp += Weight(brute[i].dis, hash_R, &bad);
      tp_map[int(brute[i].dis * 100 / 10)]++;
      ++i;
      ++j;
    } else if (cmp == 1) {
      ++j;
    } else {
      fn += Weight(brute[i].dis, hash_R, &bad);
      fn_map[int(brute[i].dis * 100 / 10)]++;
      ++i;
    }
  }
  while (i < brute.size()) {
    fn += Weight(brute[i].dis, hash_R, &bad);
    fn_map[int(brute[i].dis * 100 / 10)]++;
    ++i;
  }
  std::ofstream fout((output_file + ".accuracy.txt").c_str());
  for (int b = 0; b < 500; ++b) {
    const bool has_fn = fn_map.find(b) != fn_map.end(), has_tp = tp_map.find(b) != tp_map.end();
    if (has_fn && has_tp)
      fout << b << " " << tp_map[b] / (fn_map[b] + (double)tp_map[b]) << " " << tp_map[b] << " "
           << fn_map[b] << std::endl;
    else if (has_fn)
      fout << b << " " << 0 << " fn " << fn_map[b] << std::endl;
    else if (has_tp)
      fout << b << " " << 1 << " tp " << tp_map[b] << std::endl;
  }
  fout.close();
  if (bad) return NAN;
  return tp / (tp + fn);
}

namespace {

// An index over `points` that only serves hs_bruteforce: one table, one function (the brute-force
// scan reads the resident residue codes, not the tables).
struct ScanEngine {
  hs_handle* h = nullptr;
  uint32_t dim = 0;
  ~ScanEngine() { hs_destroy(h); }
  int Open(const std::vector<Point>& points, size_t n_points, uint32_t dim_, int device, std::string* err) {
    dim = dim_;
    std::vector<double> table;
    std::vector<uint8_t> codes;
    std::vector<Point> head;
    const std::vector<Point>* src = &points;
    if (n_points < points.size()) {
      head.assign(points.begin(), points.begin() + n_points);
      src = &head;
    }
    if (!PointsToCodes(*src, dim, &table, &codes, err)) return HS_ERR_INVALID;
    const Planes planes = DrawPlanes(dim, 1, 1, 1.0, 0);
    hs_params prm;
    memset(&prm, 0, sizeof(prm));
    prm.k = dim / 8;
    prm.K = 1;
    prm.L = 1;
    prm.W = 1.0;
    prm.device = device;
    prm.alphabet = (uint32_t)(table.size() / 8);
    hs_status st = hs_create(&prm, planes.a.data(), planes.b.data(), table.data(), &h);
    if (st != HS_OK) {
      if (err) *err = std::string("hs_create: ") + (h ? hs_last_error(h) : "no usable gfx950 device");
      return st;
    }
    st = hs_index_build(h, codes.data(), src->size());
    if (st != HS_OK && err) *err = std::string("hs_index_build: ") + hs_last_error(h);
    return st;
  }
  // all (centre, point) pairs of centres [c0, c0 + nc) with !(dist > R), centre-major
  // radii != null: centre c0 + i at radii[i] instead of R
  int Scan(const std::vector<Point>& centers, size_t c0, size_t nc, double R, std::vector<uint32_t>* hq,
           std::vector<uint32_t>* hid, std::vector<double>* hd, uint64_t* n_hits, std::string* err,
           const double* radii = nullptr) {
    std::vector<double> flat(nc * dim);
    for (size_t i = 0; i < nc; ++i) {
      if (centers[c0 + i].data.size() != dim) {
        if (err) *err = "centre with the wrong dimension";
        return HS_ERR_INVALID;
      }
      memcpy(&flat[i * dim], centers[c0 + i].data.data(), sizeof(double) * dim);
    }
    uint64_t cap = std::max<uint64_t>(hq->size(), 1024);
    for (;;) {
      hq->resize(cap);
      hid->resize(cap);
      hd->resize(cap);
      const hs_status st =
          radii ? hs_bruteforce_radii(h, flat.data(), nc, radii, hq->data(), hid->data(), hd->data(), cap, n_hits)
                : hs_bruteforce(h, flat.data(), nc, R, hq->data(), hid->data(), hd->data(), cap, n_hits);
      if (st == HS_ERR_CAPACITY) {
        cap = *n_hits;
        continue;
      }
      if (st != HS_OK && err) *err = std::string("hs_bruteforce: ") + hs_last_error(h);
      return st;
    }
  }
};

}  // namespace

int SearchBruteForce(const std::vector<Point>& kmers, const std::vector<Point>& centers,
                     const std::vector<std::string>& kmer_names,
                     const std::vector<std::string>& center_names, const double& hash_R,
                     const std::string& output_file, int device, std::string* err,
                     bool write_not_less_than, const std::vector<double>* radii) {
  if (!RadiiMatch(radii, centers.size(), err)) return HS_ERR_INVALID;
  if (kmers.empty() || kmers[0].data.empty() || kmers[0].data.size() % 8 != 0) {
    if (err) *err = "no database points (or dimension not a multiple of 8)";
    return HS_ERR_INVALID;
  }
  const uint32_t dim = (uint32_t)kmers[0].data.size();
  ScanEngine eng;
  int st = eng.Open(kmers, kmers.size(), dim, device, err);
  if (st != HS_OK) return st;
  std::ofstream fout(output_file.c_str());
  std::ofstream fnot;
  if (write_not_less_than) fnot.open((output_file + "notlessthan.txt").c_str());  // :41-43
  // with the second file every pair comes back (R = inf) and is split here by the reference's
  // test `dis > hash_R` (:47); centre blocks bound the host buffers to ~2^24 pairs
  const double R = write_not_less_than ? std::numeric_limits<double>::infinity() : hash_R;
  const size_t block = write_not_less_than
                           ? std::max<size_t>(1, (size_t)(1u << 24) / std::max<size_t>(1, kmers.size()))
                           : centers.size();
  std::vector<uint32_t> hq, hid;
  std::vector<double> hd;
  for (size_t c0 = 0; c0 < centers.size(); c0 += block) {
    const size_t nc = std::min(block, centers.size() - c0);
    uint64_t n_hits = 0;
    // (with the second file every pair comes back whatever the radii, and is split here)
    st = eng.Scan(centers, c0, nc, R, &hq, &hid, &hd, &n_hits, err,
                  radii && !write_not_less_than ? radii->data() + c0 : nullptr);
    if (st != HS_OK) return st;
    for (uint64_t i = 0; i < n_hits; ++i) {
      const double r_i = radii ? (*radii)[c0 + hq[i]] : hash_R;
      std::ofstream& f = (write_not_less_than && hd[i] > r_i) ? fnot : fout;
      f << center_names[c0 + hq[i]] << " " << kmer_names[hid[i]] << " " << hd[i] << std::endl;
    }
  }
  return HS_OK;
}

bool SortHitsFile(const std::string& hits_file, uint64_t* n_records) {
  std::ifstream fin(hits_file.c_str());
  if (!fin) return false;
  std::vector<MotifRes> rec;
  MotifRes r;
  while (fin >> r.motif >> r.protein >> r.dis) rec.push_back(r);
  std::sort(rec.begin(), rec.end(), ResLess);  // evaluate2.cpp:88
  std::ofstream fout((hits_file + "sort.txt").c_str());
  for (size_t i = 0; i < rec.size(); ++i)
    fout << rec[i].motif << "\t" << rec[i].protein << "\t" << rec[i].dis << std::endl;  // :91-93
  if (n_records) *n_records = rec.size();
  return true;
}

namespace {
// weight() of evaluate2.cpp:62-71
double Weight2(double dis) {
  if (dis > 49.38) {
    const double w = dis / (2 * 49.38);
    if (w > 1) return 1;
    return dis / (2 * 49.38);
  }
  return 1 - dis / (2 * 49.38);
}
}  // namespace

double Evaluate2(const std::string& ground_truth, const std::string& hits_file, double* tp_out,
                 double* fn_out) {
  std::vector<MotifRes> brute, found;
  MotifRes r;
  {
    std::ifstream fin(ground_truth.c_str());
    while (fin >> r.motif >> r.protein >> r.dis) brute.push_back(r);
  }
  {
    std::ifstream fin(hits_file.c_str());
    while (fin >> r.motif >> r.protein >> r.dis) found.push_back(r);
  }
  std::sort(brute.begin(), brute.end(), ResLess);   // :88
  std::sort(found.begin(), found.end(), ResLess);   // :127
  size_t i = 0, j = 0;
  double tp = 0.0, fn = 0.0;
  while (i < brute.size() && j < found.size()) {  // :131-143
    const int cmp = ResCompare(brute[i], found[j]);
    if (cmp == 0) {
      tp += Weight2(brute[i].dis);
      ++i;
      ++j;
    } else if (cmp == 1) {
      ++j;
    } else {
      fn += Weight2(brute[i].dis);
      ++i;
    }
  }
  for (; i < brute.size(); ++i) fn += Weight2(brute[i].dis);  // :144-147
  if (tp_out) *tp_out = tp;
  if (fn_out) *fn_out = fn;
  return tp / (tp + fn);
}

bool ReadMotifFamilies(const std::string& path, uint32_t min_size, std::vector<MotifFamily>* families) {
  std::ifstream fin(path.c_str());
  if (!fin) return false;
  families->clear();
  MotifFamily cur;
  std::string line;
  while (std::getline(fin, line)) {  // centerDistanceSmapling.cpp:443-453
    if (line.size() == 0) continue;
    if (line[0] == '#') {
      if (cur.seqs.size() >= min_size) families->push_back(cur);
      cur.name = line;
      cur.seqs.clear();
    } else {
      cur.seqs.push_back(line);
    }
  }
  if (cur.seqs.size() >= min_size) families->push_back(cur);  // :455-457
  return true;
}

bool FamilyCenters(const std::vector<MotifFamily>& families, uint32_t kmer_length,
                   std::vector<Point>* centers, std::string* err) {
  const uint32_t dim = 8 * kmer_length;
  centers->clear();
  for (size_t f = 0; f < families.size(); ++f) {
    Point center;
    center.data.assign(dim, 0.0);
    const std::vector<std::string>& seqs = families[f].seqs;
    for (size_t m = 0; m < seqs.size(); ++m) {
      if (seqs[m].size() != kmer_length) {
        if (err) *err = "family " + families[f].name + ": member '" + seqs[m] + "' is not a " +
                        std::to_string(kmer_length) + "-mer";
        return false;
      }
      for (uint32_t p = 0; p < kmer_length; ++p) {
        const char c = seqs[m][p];
        const int row = (c >= 'A' && c <= 'Z') ? HS_LETTER_TO_CODE[c - 'A'] : -1;
        if (row < 0) {
          if (err) *err = "family " + families[f].name + ": letter outside the 20-letter alphabet in '" + seqs[m] + "'";
          return false;
        }
        for (uint32_t j = 0; j < 8; ++j) center.data[8 * p + j] += HS_AA_COORDS[row][j];  // Center() :69-73
      }
    }
    for (uint32_t j = 0; j < dim; ++j) center.data[j] /= seqs.size();  // :74-76
    centers->push_back(center);
  }
  return true;
}

bool Cluster2DataPoint(const std::vector<MotifFamily>& families, const std::vector<Point>& centers,
                       const std::string& output_file) {
  std::ofstream fout((output_file + "hclust.format.txt").c_str());
  if (!fout) return false;
  for (size_t p = 0; p < centers.size(); ++p) {  // :126-134
    fout << families[p].name << std::endl;
    fout << centers[p].data[0];
    for (size_t q = 1; q < centers[p].data.size(); ++q) fout << " " << centers[p].data[q];
    fout << std::endl;
  }
  return true;
}

double RadiusCovering(double d2) {
  double r = sqrt(d2);
  if (r * r < d2) r = nextafter(r, std::numeric_limits<double>::infinity());
  return r;
}

bool FamilyRadii(const std::vector<MotifFamily>& families, uint32_t kmer_length, const std::string& output_file,
                 double quantile, std::string* err) {
  const uint32_t dim = 8 * kmer_length;
  if (!(quantile > 0.0 && quantile <= 1.0)) {
    if (err) *err = "the quantile must lie in (0, 1]";
    return false;
  }
  // the centroids as the points file holds them (6 significant digits): what a search is given as its centres
  std::vector<std::string> names;
  std::vector<Point> written;
  if (!ReadPointsFile(output_file + "hclust.format.txt", dim, &names, &written) || written.size() != families.size()) {
    if (err) *err = "cannot read " + output_file + "hclust.format.txt back";
    return false;
  }
  std::ofstream fout((output_file + "hclust.radii.txt").c_str());
  if (!fout) {
    if (err) *err = "cannot write " + output_file + "hclust.radii.txt";
    return false;
  }
  for (size_t f = 0; f < families.size(); ++f) {
    const std::vector<std::string>& seqs = families[f].seqs;
    std::vector<double> d2s;
    for (size_t m = 0; m < seqs.size(); ++m) {  // (letters and lengths were checked by FamilyCenters)
      double d2 = 0.0;  // PairwiseDistance_square: left to right
      for (uint32_t p = 0; p < kmer_length; ++p) {
        const int row = HS_LETTER_TO_CODE[seqs[m][p] - 'A'];
        for (uint32_t j = 0; j < 8; ++j) {
          const double r = HS_AA_COORDS[row][j] - written[f].data[8 * p + j];
          d2 += r * r;
        }
      }
      d2s.push_back(d2);
    }
    std::sort(d2s.begin(), d2s.end());
    // nearest rank: the smallest member distance that at least quantile x n of the members do not exceed
    size_t rank = (size_t)ceil(quantile * (double)d2s.size());
    rank = std::min(std::max<size_t>(rank, 1), d2s.size());
    char num[64];
    snprintf(num, sizeof(num), "%.17g", RadiusCovering(d2s[rank - 1]));
    fout << families[f].name << " " << num << std::endl;
  }
  return true;
}

bool ReadRadiiFile(const std::string& path, const std::vector<std::string>& center_names,
                   std::vector<double>* radii, std::string* err) {
  std::ifstream fin(path.c_str());
  if (!fin) {
    if (err) *err = "cannot open " + path;
    return false;
  }
  std::unordered_map<std::string, size_t> index;
  for (size_t i = 0; i < center_names.size(); ++i)
    if (!index.insert(std::make_pair(center_names[i], i)).second) {
      if (err) *err = "radii: centre name '" + center_names[i] + "' is not unique in the centres file";
      return false;
    }
  radii->assign(center_names.size(), 0.0);
  std::vector<char> seen(center_names.size(), 0);
  std::string line;
  size_t line_no = 0;
  const char* ws = " \t\r";
  while (std::getline(fin, line)) {
    ++line_no;
    const size_t last = line.find_last_not_of(ws);
    if (last == std::string::npos) continue;  // blank line
    line.erase(last + 1);
    const std::string where = path + ":" + std::to_string(line_no) + ": ";
    const size_t gap = line.find_last_of(ws);
    const size_t name_end = gap == std::string::npos ? std::string::npos : line.find_last_not_of(ws, gap);
    if (name_end == std::string::npos) {
      if (err) *err = where + "expected '<centre name> <radius>'";
      return false;
    }
    const std::string name = line.substr(0, name_end + 1), number = line.substr(gap + 1);
    char* end = nullptr;
    errno = 0;
    const double r = strtod(number.c_str(), &end);
    if (end == number.c_str() || *end != '\0' || !(r == r)) {
      if (err) *err = where + "'" + number + "' is not a radius";
      return false;
    }
    const auto it = index.find(name);
    if (it == index.end()) {
      if (err) *err = where + "'" + name + "' is not a centre";
      return false;
    }
    if (seen[it->second]) {
      if (err) *err = where + "centre '" + name + "' has a radius already";
      return false;
    }
    seen[it->second] = 1;
    (*radii)[it->second] = r;
  }
  for (size_t i = 0; i < seen.size(); ++i)
    if (!seen[i]) {
      if (err) *err = path + ": no radius for centre '" + center_names[i] + "'";
      return false;
    }
  return true;
}

int SequenceDatabase2Centers(const std::vector<Point>& kmers_proteins,
                             const std::vector<Point>& centers, const std::string& output_file,
                             const std::string& dir, int device, std::string* err) {
  if (centers.empty() || kmers_proteins.empty()) {
    if (err) *err = "no centres or no database points";
    return HS_ERR_INVALID;
  }
  const uint32_t dim = (uint32_t)centers[0].data.size();
  if (mkdir(dir.c_str(), 0777) != 0 && errno != EEXIST) {
    if (err) *err = "cannot create " + dir;
    return HS_ERR_IO;
  }
  {
    // :152-161 -- PairwiseDistance (:58-65): sequential fp64, sqrt
    std::ofstream fcenter((dir + "/" + output_file + "innercenter_protein_centers_0.txt").c_str());
    if (!fcenter) {
      if (err) *err = "cannot write into " + dir;
      return HS_ERR_IO;
    }
    for (size_t i = 0; i < centers.size(); ++i)
      for (size_t j = i + 1; j < centers.size(); ++j) {
        double dis = 0.0;
        for (uint32_t t = 0; t < dim; ++t) {
          const double r = centers[i].data[t] - centers[j].data[t];
          dis += r * r;
        }
        fcenter << sqrt(dis) << std::endl;
      }
  }
  const size_t n_sample = std::min<size_t>(100000, kmers_proteins.size());  // :166-173
  ScanEngine eng;
  int st = eng.Open(kmers_proteins, n_sample, dim, device, err);
  if (st != HS_OK) return st;
  std::ofstream fout((dir + "/" + output_file + "ramdom_protein_centers_0.txt").c_str());
  std::vector<uint32_t> hq, hid;
  std::vector<double> hd;
  const size_t block = std::max<size_t>(1, (size_t)(1u << 24) / n_sample);
  for (size_t c0 = 0; c0 < centers.size(); c0 += block) {  // :178-182, centre-major
    const size_t nc = std::min(block, centers.size() - c0);
    uint64_t n_hits = 0;
    st = eng.Scan(centers, c0, nc, std::numeric_limits<double>::infinity(), &hq, &hid, &hd, &n_hits, err);
    if (st != HS_OK) return st;
    if (n_hits != (uint64_t)nc * n_sample) {
      if (err) *err = "brute-force scan returned an incomplete distance matrix";
      return HS_ERR_STATE;
    }
    for (uint64_t i = 0; i < n_hits; ++i) fout << hd[i] << std::endl;
  }
  return HS_OK;
}

}  // namespace hsearch
