// hs_hclust2.cpp -- the `hclust2` program of the reference on the GPU path.
//
// Keeps the reference's command line (hclust/src/hclust/hclust2.cpp:199-213):
//     -k <kmers.fa> -l <k> -K <hash_K> -L <hash_L> -W <w> -T <R> -o <out>
// (also -kmers/-len/-hash_K/-hash_L/-window/-threshold/-output) and its exit behaviour (missing
// option -> help, exit 0, :223-226; runtime error -> stderr, exit 1).  Additions: --seed (planes
// drawn like the reference's LSH constructor, table l seeded seed + l; default random_device as
// the reference), --device, and -linkage greedy|single|dbscan|density (-M; density: the end of this comment): `single` writes the connected components of the
// near-neighbour graph (hsearch::Components) in place of the greedy leader clusters, `dbscan` its density clusters
// (hsearch::Dbscan) at -minpts M (-p; required with dbscan, an error without it); the default is the reference's.
// -centers 1 (-C; with -linkage single or dbscan only) writes beside the clusters file the centroids of the clusters
// of at least -minsize m (-m, default 50: the reference's MIN_SIZE_CLUSTER) members as <o>hclust.format.txt and their
// covering radii as <o>hclust.radii.txt (hsearch::ClusterCenters): the -c / --radii inputs of hs_motif_both_points.
// -tree 1 (-t; with -linkage single only) writes beside the clusters file the single-linkage tree up to the threshold
// as <o>hclust.tree.txt (hsearch::SingleLinkageTree): one line per merge, in merge order.
// -linkage density -minpts M (hsearch::DensityTree): the clusters file holds the DBSCAN* clusters at the threshold
// (dbscan's without their border k-mers), <o>hclust.core.txt every k-mer's core distance; with it -tree 1 writes the
// density tree -- DBSCAN at every radius up to the threshold -- in the same format, and -centers 1 works as for dbscan.
// -knn N (-n; 1..64, with -linkage single, dbscan or density) writes beside the clusters file the k-nearest-neighbour
// graph within the threshold as <o>hclust.knn.txt (hsearch::KnnGraph): one line per k-mer -- its name, its degree, then
// its at most N nearest neighbours as name / distance pairs.
// -pssm 1 (-P; wherever -centers 1 works) writes beside the clusters file the profiles of the clusters of at least
// -minsize m members as <o>hclust.pssm.txt (hsearch::ClusterProfiles): the --pssm input of hs_motif_both_points, which
// then reports every member of every cluster under its cluster's name.  -pssm-weights none|sites|columns (-w, default
// sites): raw counts, or position-based sequence weights scaled to the members / to the distinct residues per column;
// -pssm-threshold cover|rank (-H, default cover): the covering threshold, or the score of the size-th best k-mer;
// -pssm-pseudo x (-u, default 1): pseudo-counts of the log-odds.
#include <stdio.h>
#include <stdlib.h>
#include <time.h>

#include <iostream>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "hs_host.hpp"

namespace {
struct Opt {
  const char* long_name;
  char short_name;
  const char* descr;
  bool required;
};
const Opt kOpts[] = {
    {"kmers", 'k', "kmers file", true},
    {"len", 'l', "kmer length", true},
    {"hash_K", 'K', "number of random lines", true},
    {"hash_L", 'L', "number of hash tables", true},
    {"window", 'W', "bucket width", true},
    {"threshold", 'T', "clustering threshold", true},
    {"output", 'o', "output file name", true},
    {"seed", 's', "seed of the LSH planes [random_device]", false},
    {"device", 'G', "GPU ordinal [0]", false},
    {"linkage", 'M', "greedy (the reference's leader clusters) | single (connected components) | dbscan (density "
                     "clusters, needs -minpts) | density (the density tree: dbscan at every radius up to the "
                     "threshold, needs -minpts; writes <output>hclust.core.txt) [greedy]", false},
    {"minpts", 'p', "dbscan: neighbours within the threshold, the k-mer itself counted, that make a k-mer dense", false},
    {"centers", 'C', "1: also write <output>hclust.format.txt (centroids) and <output>hclust.radii.txt (covering radii) "
                     "of the clusters; with -linkage single or dbscan [0]", false},
    {"minsize", 'm', "centers, pssm: members a cluster needs to get a centre or a profile [50]", false},
    {"pssm", 'P', "1: also write <output>hclust.pssm.txt, the clusters' profiles with thresholds (the --pssm input of "
                  "hs_motif_both_points); with -linkage single, dbscan or density [0]", false},
    {"pssm-weights", 'w', "pssm: none (raw counts) | sites | columns (position-based sequence weights, scaled to the "
                          "members | to the distinct residues per column) [sites]", false},
    {"pssm-threshold", 'H', "pssm: cover (every member of a cluster is a hit of its profile) | rank (the score of the "
                            "profile's size-th best k-mer) [cover]", false},
    {"pssm-pseudo", 'u', "pssm: pseudo-counts of the log-odds, > 0 [1]", false},
    {"tree", 't', "1: also write <output>hclust.tree.txt, the single-linkage tree up to the threshold, one line per "
                  "merge in merge order: two k-mer names and the distance; with -linkage single [0]", false},
    {"knn", 'n', "N (1..64): also write <output>hclust.knn.txt, per k-mer its name, its number of neighbours within the "
                 "threshold and its N nearest as name / distance pairs; with -linkage single, dbscan or density [off]", false},
};
void Help(const char* prog) {
  fprintf(stderr, "Usage: %s [OPTIONS]\n\nOptions:\n", prog);
  for (const Opt& o : kOpts)
    fprintf(stderr, "  -%c, -%-12s %s%s\n", o.short_name, o.long_name, o.descr,
            o.required ? " [REQUIRED]" : "");
  fprintf(stderr, "\nHelp options:\n  -?, -help   print this help message\n\ncluster kmers to motifs\n");
}
}  // namespace

int main(int argc, const char* argv[]) {
  bool help = false;
  std::map<std::string, std::string> val;
  for (int i = 1; i < argc; ++i) {
    std::string arg = argv[i];
    if (arg == "-help" || arg == "--help" || arg == "-?" || arg == "-about") {
      help = true;
      continue;
    }
    if (arg.size() < 2 || arg[0] != '-') continue;
    std::string name = arg.substr(arg[1] == '-' ? 2 : 1);
    const Opt* hit = nullptr;
    for (const Opt& o : kOpts)
      if (name == o.long_name || (name.size() == 1 && name[0] == o.short_name)) hit = &o;
    if (!hit) {
      fprintf(stderr, "unknown option %s\n", arg.c_str());
      return EXIT_FAILURE;
    }
    if (i + 1 >= argc) {
      fprintf(stderr, "option %s needs a value\n", arg.c_str());
      return EXIT_FAILURE;
    }
    val[hit->long_name] = argv[++i];
  }
  if (argc > 1 && !help) {
    fprintf(stdout, "[WELCOME TO PMF v1.0 -- MI355X]\n[%s", argv[0]);
    for (int i = 1; i < argc; ++i) fprintf(stdout, " %s", argv[i]);
    fprintf(stdout, "]\n");
  }
  if (argc == 1 || help) {
    Help(argv[0]);
    return EXIT_SUCCESS;
  }
  for (const Opt& o : kOpts)
    if (o.required && !val.count(o.long_name)) {
      fprintf(stderr, "missing required option -%c\n", o.short_name);
      Help(argv[0]);
      return EXIT_SUCCESS;
    }
  const uint32_t len = (uint32_t)strtoul(val["len"].c_str(), nullptr, 10);
  const uint32_t hash_K = (uint32_t)strtoul(val["hash_K"].c_str(), nullptr, 10);
  const uint32_t hash_L = (uint32_t)strtoul(val["hash_L"].c_str(), nullptr, 10);
  const double hash_W = strtod(val["window"].c_str(), nullptr);
  const double hash_R = strtod(val["threshold"].c_str(), nullptr);
  const int device = val.count("device") ? atoi(val["device"].c_str()) : 0;
  const std::string linkage = val.count("linkage") ? val["linkage"] : "greedy";
  const bool density = linkage == "density";
  if (linkage != "greedy" && linkage != "single" && linkage != "dbscan" && !density) {
    fprintf(stderr, "ERROR: -linkage must be greedy, single, dbscan or density, not '%s'\n", linkage.c_str());
    return EXIT_FAILURE;
  }
  if (density && !val.count("minpts")) {
    fprintf(stderr, "ERROR: -linkage density needs -minpts\n");
    return EXIT_FAILURE;
  }
  if (!density && (linkage == "dbscan") != (val.count("minpts") != 0)) {
    fprintf(stderr, linkage == "dbscan" ? "ERROR: -linkage dbscan needs -minpts\n"
                                        : "ERROR: -minpts goes with -linkage dbscan only\n");
    return EXIT_FAILURE;
  }
  uint32_t min_pts = 0;
  if (linkage == "dbscan" || density) {
    char* end = nullptr;
    const unsigned long long m = strtoull(val["minpts"].c_str(), &end, 10);
    if (end == val["minpts"].c_str() || *end || m < 1 || m > 0xffffffffull || val["minpts"][0] == '-') {
      fprintf(stderr, "ERROR: -minpts must be a whole number of at least 1, not '%s'\n", val["minpts"].c_str());
      return EXIT_FAILURE;
    }
    min_pts = (uint32_t)m;
  }
  uint32_t centers_min_size = 0;  // 0: no centres
  if (val.count("centers") && val["centers"] != "0" && val["centers"] != "1") {
    fprintf(stderr, "ERROR: -centers takes 0 or 1, not '%s'\n", val["centers"].c_str());
    return EXIT_FAILURE;
  }
  const bool centers = val.count("centers") && val["centers"] == "1";
  if (centers && linkage == "greedy") {
    fprintf(stderr, "ERROR: -centers goes with -linkage single or dbscan, not with the greedy leader clusters\n");
    return EXIT_FAILURE;
  }
  if (val.count("pssm") && val["pssm"] != "0" && val["pssm"] != "1") {
    fprintf(stderr, "ERROR: -pssm takes 0 or 1, not '%s'\n", val["pssm"].c_str());
    return EXIT_FAILURE;
  }
  const bool pssm = val.count("pssm") && val["pssm"] == "1";
  if (pssm && linkage == "greedy") {
    fprintf(stderr, "ERROR: -pssm goes with -linkage single, dbscan or density, not with the greedy leader clusters\n");
    return EXIT_FAILURE;
  }
  for (const char* name : {"pssm-weights", "pssm-threshold", "pssm-pseudo"})
    if (val.count(name) && !pssm) {
      fprintf(stderr, "ERROR: -%s goes with -pssm 1 only\n", name);
      return EXIT_FAILURE;
    }
  if (val.count("minsize") && !centers && !pssm) {
    fprintf(stderr, "ERROR: -minsize goes with -centers 1 only\n");
    return EXIT_FAILURE;
  }
  uint32_t min_size = 50;  // MIN_SIZE_CLUSTER, centerDistanceSmapling.cpp:12
  if (val.count("minsize")) {
    char* end = nullptr;
    const unsigned long long m = strtoull(val["minsize"].c_str(), &end, 10);
    if (end == val["minsize"].c_str() || *end || m < 1 || m > 0xffffffffull || val["minsize"][0] == '-') {
      fprintf(stderr, "ERROR: -minsize must be a whole number of at least 1, not '%s'\n", val["minsize"].c_str());
      return EXIT_FAILURE;
    }
    min_size = (uint32_t)m;
  }
  if (centers) centers_min_size = min_size;
  hsearch::ClusterProfileOptions profiles;  // min_size 0: no profiles
  if (pssm) {
    profiles.min_size = min_size;
    const std::string w = val.count("pssm-weights") ? val["pssm-weights"] : "sites";
    const std::string th = val.count("pssm-threshold") ? val["pssm-threshold"] : "cover";
    if (w != "none" && w != "sites" && w != "columns") {
      fprintf(stderr, "ERROR: -pssm-weights must be none, sites or columns, not '%s'\n", w.c_str());
      return EXIT_FAILURE;
    }
    if (th != "cover" && th != "rank") {
      fprintf(stderr, "ERROR: -pssm-threshold must be cover or rank, not '%s'\n", th.c_str());
      return EXIT_FAILURE;
    }
    profiles.weights = w == "none" ? 0 : w == "sites" ? 1 : 2;
    profiles.threshold = th == "cover" ? 0 : 1;
    if (val.count("pssm-pseudo")) {
      char* end = nullptr;
      profiles.pseudo = strtod(val["pssm-pseudo"].c_str(), &end);
      if (end == val["pssm-pseudo"].c_str() || *end || !(profiles.pseudo > 0.0) ||
          !(profiles.pseudo <= 1.7976931348623157e308)) {
        fprintf(stderr, "ERROR: -pssm-pseudo takes a finite number above 0\n");
        return EXIT_FAILURE;
      }
    }
  }
  if (val.count("tree") && val["tree"] != "0" && val["tree"] != "1") {
    fprintf(stderr, "ERROR: -tree takes 0 or 1, not '%s'\n", val["tree"].c_str());
    return EXIT_FAILURE;
  }
  const bool tree = val.count("tree") && val["tree"] == "1";
  if (tree && linkage != "single" && !density) {
    fprintf(stderr, "ERROR: -tree goes with -linkage single only: the tree is the single-linkage tree\n");
    return EXIT_FAILURE;
  }
  uint32_t knn = 0;  // 0: no graph file
  if (val.count("knn")) {
    if (linkage == "greedy") {
      fprintf(stderr, "ERROR: -knn goes with -linkage single, dbscan or density, not with the greedy leader clusters\n");
      return EXIT_FAILURE;
    }
    char* end = nullptr;
    const unsigned long long m = strtoull(val["knn"].c_str(), &end, 10);
    if (end == val["knn"].c_str() || *end || m < 1 || m > 64 || val["knn"][0] == '-') {
      fprintf(stderr, "ERROR: -knn must be a whole number 1..64, not '%s'\n", val["knn"].c_str());
      return EXIT_FAILURE;
    }
    knn = (uint32_t)m;
  }
  uint32_t seed;
  if (val.count("seed")) {
    seed = (uint32_t)strtoul(val["seed"].c_str(), nullptr, 10);
  } else {
    std::random_device rd;
    seed = rd();
  }
  try {
    std::vector<hsearch::Kmer> kmers;
    if (!hsearch::ReadKmerFasta(val["kmers"], &kmers)) {
      fprintf(stderr, "cannot open %s\n", val["kmers"].c_str());
      return EXIT_FAILURE;
    }
    printf("The number of kmers is %zu\n", kmers.size());
    const hsearch::Planes planes = hsearch::DrawPlanes(8 * len, hash_K, hash_L, hash_W, seed);
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    std::cout << "Clustering... " << std::endl;
    std::string err;
    uint64_t n_clusters = 0;
    const int st = density
                       ? hsearch::DensityTree(kmers, hash_K, hash_L, hash_W, hash_R, min_pts, val["output"], planes,
                                              device, &err, tree, &n_clusters, nullptr, seed, centers_min_size,
                                              &profiles)
                   : linkage == "dbscan"
                       ? hsearch::Dbscan(kmers, hash_K, hash_L, hash_W, hash_R, min_pts, val["output"], planes, device,
                                         &err, &n_clusters, seed, centers_min_size, &profiles)
                   : tree
                       ? hsearch::SingleLinkageTree(kmers, hash_K, hash_L, hash_W, hash_R, val["output"], planes, device,
                                                    &err, &n_clusters, nullptr, seed, centers_min_size, &profiles)
                   : linkage == "single"
                       ? hsearch::Components(kmers, hash_K, hash_L, hash_W, hash_R, val["output"], planes, device, &err,
                                             &n_clusters, seed, centers_min_size, &profiles)
                       : hsearch::Clustering(kmers, hash_K, hash_L, hash_W, hash_R, val["output"], planes, device, seed,
                                             &err, &n_clusters);
    if (st != 0) {
      fprintf(stderr, "ERROR: %s (status %d)\n", err.c_str(), st);
      return EXIT_FAILURE;
    }
    if (knn) {
      uint64_t n_edges = 0;
      const int kst = hsearch::KnnGraph(kmers, hash_K, hash_L, hash_W, hash_R, knn, val["output"], planes, device, &err,
                                        &n_edges, seed);
      if (kst != 0) {
        fprintf(stderr, "ERROR: %s (status %d)\n", err.c_str(), kst);
        return EXIT_FAILURE;
      }
      printf("knn_graph_edges = %llu\n", (unsigned long long)n_edges);
    }
    clock_gettime(CLOCK_MONOTONIC, &t1);
    printf("num_of_clusters = %llu\n", (unsigned long long)n_clusters);
    printf("Clustering takes %lf seconds\n", (t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec));
  } catch (const std::bad_alloc&) {
    fprintf(stderr, "ERROR: could not allocate memory\n");
    return EXIT_FAILURE;
  } catch (const std::exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return EXIT_FAILURE;
  }
  return EXIT_SUCCESS;
}
