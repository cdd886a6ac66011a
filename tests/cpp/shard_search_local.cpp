// Pose search over a sharded filter through the C++ adapter: badger_amcl_amd::LocalShardedParticleFilter over `world`
// engines on GPU 0, each with the map, the scanner and a filter of its own.  The exhaustive and the pruned search
// over the whole space go to files as raw bpf_pose_hit rows, then localize() runs and the ranks' slices go to a third
// file in rank order, for tests/test_gpu_cpp_shard_search.py to compare with the Python side.  Input arrays come from
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

static void dump(const char* path, const void* p, size_t bytes)
{
  FILE* f = std::fopen(path, "wb");
  if (!f) { std::perror(path); std::exit(2); }
  std::fwrite(p, 1, bytes, f);
  std::fclose(f);
}

int main(int argc, char** argv)
{
  if (argc < 20)
  {
    std::fprintf(stderr, "usage: cells lut ranges angles size_x size_y res origin_x origin_y max_beams headings stride k "
                         "block world samples out_exhaustive out_pruned out_sets\n");
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
  const int k = std::atoi(argv[13]), block = std::atoi(argv[14]), W = std::atoi(argv[15]), n = std::atoi(argv[16]);
  try
  {
    std::vector<std::shared_ptr<OccupancyMap>> maps;
    std::vector<std::shared_ptr<PlanarScanner>> scanners;
    std::vector<std::shared_ptr<ParticleFilter>> pfs;
    for (int r = 0; r < W; ++r)
    {
      auto eng = std::make_shared<Engine>(0);
      auto map = std::make_shared<OccupancyMap>(eng, res);
      map->setSize({ size_x, size_y });
      map->setOrigin(origin_x, origin_y);
      for (int i = 0; i < size_x * size_y; ++i)
        map->setCellState(i, (MapCellState)cells[i]);
      map->setDistancesLUT(lut, 2.0);
      auto scanner = std::make_shared<PlanarScanner>(eng);
      scanner->init(max_beams, map);
      scanner->setModelLikelihoodField(0.95, 0.05, 0.2, 2.0);
      scanner->setMapFactors(0.95, 0.95, 0.3);
      scanner->setPlanarScannerPose({ 0.1, -0.05, 0.2 });
      auto pf = std::make_shared<ParticleFilter>(eng, 100, n, 0.0, 0.0, 85.0);
      pf->srand48(7);
      maps.push_back(map);
      scanners.push_back(scanner);
      pfs.push_back(pf);
    }
    LocalShardedParticleFilter local(pfs);

    auto data = std::make_shared<PlanarData>();
    data->range_count_ = (int)ranges.size();
    data->range_max_ = 30.0;
    data->ranges_ = ranges;
    data->angles_ = angles;

    const auto rows = local.searchPoses(data, headings, stride, k);
    dump(argv[17], rows.data(), rows.size() * sizeof(bpf_pose_hit));
    std::vector<bpf_pose_search_stats> stats;
    const auto pruned = local.searchPosesPruned(data, headings, stride, k, block, 0, -1, &stats);
    dump(argv[18], pruned.data(), pruned.size() * sizeof(bpf_pose_hit));
    long long candidates = 0, scored = 0;
    for (const auto& st : stats)
    {
      candidates += st.candidates;
      scored += st.scored_candidates;
    }
    // a range inside the space, cut by first / count
    const auto part = local.searchPoses(data, headings, stride, k, 11, 70000);

    ShardedParticleFilter::LocalizeSettings s;
    s.refine_xy_step = s.moments_xy_step = res / 2;
    s.block = block;
    const auto comps = local.localize(scanners, data, headings, stride, k, s);
    std::vector<PFSample> whole;
    std::vector<std::vector<PFSample>> sets((size_t)W);
    local.forEachRank([&](int r, ParticleFilter& pf) { sets[(size_t)r] = pf.getCurrentSet()->samples; });
    for (const auto& set : sets)
      whole.insert(whole.end(), set.begin(), set.end());
    dump(argv[19], whole.data(), whole.size() * sizeof(PFSample));
    std::printf("%zu %zu %zu %lld %lld %zu %zu\n", rows.size(), pruned.size(), part.size(), candidates, scored,
                comps.size(), whole.size());
    local.shutdown();
  }
  catch (const std::exception& err)
  {
    std::fprintf(stderr, "shard_search_local: %s\n", err.what());
    return 1;
  }
  return 0;
}
