// The pruned cloud pose search through the C++ adapter's OctoMap / PointCloudScanner: the whole block list in one
// call with its stats, the exhaustive search of the same space, the block list as three ranges (cut at the two block
// indices given) whose hit lists PointCloudScanner::mergePoseHits folds, the bounds and the pooled volume.  The
// results go to files (raw bpf_pose_hit rows, doubles, bytes) for the Python test to compare.  Input arrays come from
// binary files written by the test (so both sides see identical bits).
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "badger_amcl_amd/adapter.hpp"

using namespace badger_amcl_amd;

template <typename T>
static std::vector<T> slurp(const char* path)
{
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::perror(path); std::exit(2); }
  std::fseek(f, 0, SEEK_END);
  const long n = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<T> v(n / sizeof(T));
  if (std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) std::exit(2);
  std::fclose(f);
  return v;
}

template <typename T>
static void dump(const char* path, const std::vector<T>& rows)
{
  FILE* f = std::fopen(path, "wb");
  if (!f) { std::perror(path); std::exit(2); }
  std::fwrite(rows.data(), sizeof(T), rows.size(), f);
  std::fclose(f);
}

int main(int argc, char** argv)
{
  if (argc < 21)
  {
    std::fprintf(stderr, "usage: pose_indices ratios cells6 points tf7 res max_dist max_beams gompertz headings stride "
                         "k block cut1 cut2 out_pruned out_exhaustive out_merged out_bounds out_pooled\n");
    return 2;
  }
  auto pose_indices = slurp<uint32_t>(argv[1]);
  auto ratios = slurp<uint8_t>(argv[2]);
  auto cells = slurp<int32_t>(argv[3]);  // min i j k, max i j k
  auto points = slurp<float>(argv[4]);
  auto tf = slurp<double>(argv[5]);      // x y z, quaternion x y z w
  if (cells.size() != 6 || tf.size() != 7) { std::fprintf(stderr, "cells6 / tf7 sizes\n"); return 2; }
  const double res = std::atof(argv[6]), max_dist = std::atof(argv[7]);
  const int max_beams = std::atoi(argv[8]), gompertz = std::atoi(argv[9]);
  const int headings = std::atoi(argv[10]), stride = std::atoi(argv[11]), k = std::atoi(argv[12]);
  const int block = std::atoi(argv[13]), cut1 = std::atoi(argv[14]), cut2 = std::atoi(argv[15]);

  auto eng = std::make_shared<Engine>(0);
  auto map = std::make_shared<OctoMap>(eng, res);
  map->setDistancesLUT(pose_indices, ratios, { cells[0], cells[1], cells[2] }, { cells[3], cells[4], cells[5] },
                       max_dist);
  auto scanner = std::make_shared<PointCloudScanner>(eng);
  scanner->init(max_beams, map);
  if (gompertz)
    scanner->setPointCloudModelGompertz(0.5, 0.5, 0.1, 0.748, 5.0, 1.2, -3.2, 6.7, 0.25);
  else
    scanner->setPointCloudModel(0.5, 0.05, 0.1);
  scanner->setMapFactors(0.95, 0.95, 0.3);
  scanner->setPointCloudScannerToFootprintTF({ tf[0], tf[1], tf[2] }, { tf[3], tf[4], tf[5], tf[6] });

  auto data = std::make_shared<PointCloudData>();
  data->points_ = points;

  const int nb = scanner->searchBlocks(stride, block);
  if (!(0 < cut1 && cut1 < cut2 && cut2 < nb)) { std::fprintf(stderr, "cuts outside the %d blocks\n", nb); return 3; }
  bpf_pose_search_stats st{};
  dump(argv[16], scanner->searchPosesPruned(data, headings, stride, k, block, 0, -1, &st));
  dump(argv[17], scanner->searchPoses(data, headings, stride, k));
  std::vector<std::vector<bpf_pose_hit>> parts;
  parts.push_back(scanner->searchPosesPruned(data, headings, stride, k, block, 0, cut1));
  parts.push_back(scanner->searchPosesPruned(data, headings, stride, k, block, cut1, cut2 - cut1));
  parts.push_back(scanner->searchPosesPruned(data, headings, stride, k, block, cut2, -1));
  dump(argv[18], PointCloudScanner::mergePoseHits(parts, k));
  dump(argv[19], scanner->searchBounds(data, headings, stride, block));
  int ntx = 0, nty = 0, planes = 0;
  dump(argv[20], scanner->searchPooledLut(block, &ntx, &nty, &planes));
  std::printf("%d %d %d %d %lld %lld %lld %lld %lld %lld %lld\n", nb, ntx, nty, planes, st.candidates,
              st.block_candidates, st.seed_candidates, st.pruned_block_candidates, st.expanded_block_candidates,
              st.scored_candidates, st.windows);
  return 0;
}
