// The exhaustive pose search through the C++ adapter: the whole candidate space in one call, and the same space as
// three ranges (cut at the two indices given) whose hit lists PlanarScanner::mergePoseHits folds.  Both results go to
// files as raw bpf_pose_hit rows for the Python test to compare.  Input arrays come from binary files written by the
// test (so both sides see identical bits).
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
  if (argc < 18)
  {
    std::fprintf(stderr, "usage: cells lut ranges angles size_x size_y res origin_x origin_y max_beams headings stride k "
                         "cut1 cut2 out_whole out_merged\n");
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
  const int k = std::atoi(argv[13]);
  const long long cut1 = std::atoll(argv[14]), cut2 = std::atoll(argv[15]);

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

  int free_cells = 0;
  const long long total = scanner->searchSpace(headings, stride, &free_cells);
  if (!(0 < cut1 && cut1 < cut2 && cut2 < total)) { std::fprintf(stderr, "cuts outside the space of %lld\n", total); return 3; }
  dump(argv[16], scanner->searchPoses(data, headings, stride, k));
  std::vector<std::vector<bpf_pose_hit>> parts;
  parts.push_back(scanner->searchPoses(data, headings, stride, k, 0, cut1));
  parts.push_back(scanner->searchPoses(data, headings, stride, k, cut1, cut2 - cut1));
  parts.push_back(scanner->searchPoses(data, headings, stride, k, cut2));
  dump(argv[17], PlanarScanner::mergePoseHits(parts, k));
  std::printf("%lld %d %zu %zu %zu\n", total, free_cells, parts[0].size(), parts[1].size(), parts[2].size());
  return 0;
}
