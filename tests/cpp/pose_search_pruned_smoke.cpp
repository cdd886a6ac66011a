// The pruned pose search through the C++ adapter: the whole block list in one call with its stats, the exhaustive
// search of the same space, and the block list as three ranges (cut at the two block indices given) whose hit lists
// PlanarScanner::mergePoseHits folds.  The three results go to files as raw bpf_pose_hit rows for the Python test to
// compare.  Input arrays come from binary files written by the test (so both sides see identical bits).
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

static void dump(const char* path, const std::vector<bpf_pose_hit>& hits)
{
  FILE* f = std::fopen(path, "wb");
  if (!f) { std::perror(path); std::exit(2); }
  std::fwrite(hits.data(), sizeof(bpf_pose_hit), hits.size(), f);
  std::fclose(f);
}

int main(int argc, char** argv)
{
  if (argc < 20)
  {
    std::fprintf(stderr, "usage: cells lut ranges angles size_x size_y res origin_x origin_y max_beams headings stride k "
                         "block cut1 cut2 out_pruned out_exhaustive out_merged\n");
    return 2;
  }
  auto cells = slurp<int32_t>(argv[1]);
  auto lut = slurp<float>(argv[2]);
  auto ranges = slurp<double>(argv[3]);
  auto angles = slurp<double>(argv[4]);
  const int size_x = std::atoi(argv[5]), size_y = std::atoi(argv[6]);
  const double res = std::atof(argv[7]);
  const float origin_x = (float)std::atof(argv[8]), origin_y = (float)std::atof(argv[9]);
  const int max_beams = std::atoi(argv[10]), headings = std::atoi(argv[11]), stride = std::atoi(argv[12]);
  const int k = std::atoi(argv[13]), block = std::atoi(argv[14]);
  const int cut1 = std::atoi(argv[15]), cut2 = std::atoi(argv[16]);

  auto eng = std::make_shared<Engine>(0);
  auto map = std::make_shared<OccupancyMap>(eng, res);
  map->setSize({ size_x, size_y });
  map->setOrigin(origin_x, origin_y);
  for (int i = 0; i < size_x * size_y; ++i)
    map->setCellState(i, (MapCellState)cells[i]);
  map->setDistancesLUT(lut, 2.0);

  // no ParticleFilter: the search needs the map, its LUT and a planar model only
  auto scanner = std::make_shared<PlanarScanner>(eng);
  scanner->init(max_beams, map);
  scanner->setModelLikelihoodField(0.95, 0.05, 0.2, 2.0);
  scanner->setMapFactors(0.95, 0.95, 0.3);
  scanner->setPlanarScannerPose({ 0.1, -0.05, 0.2 });

  auto data = std::make_shared<PlanarData>();
  data->range_count_ = (int)ranges.size();
  data->range_max_ = 30.0;
  data->ranges_ = ranges;
  data->angles_ = angles;

  const int n_blocks = scanner->searchBlocks(stride, block);
  if (!(0 < cut1 && cut1 < cut2 && cut2 < n_blocks)) { std::fprintf(stderr, "cuts outside the %d blocks\n", n_blocks); return 3; }
  bpf_pose_search_stats st{};
  dump(argv[17], scanner->searchPosesPruned(data, headings, stride, k, block, 0, -1, &st));
  dump(argv[18], scanner->searchPoses(data, headings, stride, k));
  std::vector<std::vector<bpf_pose_hit>> parts;
  parts.push_back(scanner->searchPosesPruned(data, headings, stride, k, block, 0, cut1));
  parts.push_back(scanner->searchPosesPruned(data, headings, stride, k, block, cut1, cut2 - cut1));
  parts.push_back(scanner->searchPosesPruned(data, headings, stride, k, block, cut2));
  dump(argv[19], PlanarScanner::mergePoseHits(parts, k));
  std::printf("%d %lld %lld %lld %lld %lld %lld %lld\n", n_blocks, st.candidates, st.block_candidates, st.seed_candidates,
              st.pruned_block_candidates, st.expanded_block_candidates, st.scored_candidates, st.windows);
  return 0;
}
