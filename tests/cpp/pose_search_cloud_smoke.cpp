// The exhaustive pose search with the cloud scanner through the C++ adapter's OctoMap / PointCloudScanner: the whole
// candidate space in one call, the same space as three ranges (cut at the two indices given) whose hit lists
// PointCloudScanner::mergePoseHits folds, and applyModelToSampleSet on the samples given.  The results go to files
// (raw bpf_pose_hit rows, raw PFSample records) for the Python test to compare.  Input arrays come from binary files
// written by the test (so both sides see identical bits).
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
    std::fprintf(stderr, "usage: pose_indices ratios cells6 points samples tf7 res max_dist max_beams gompertz headings "
                         "stride k cut1 cut2 out_whole out_merged out_samples out_total out_lut\n");
    return 2;
  }
  auto pose_indices = slurp<uint32_t>(argv[1]);
  auto ratios = slurp<uint8_t>(argv[2]);
  auto cells = slurp<int32_t>(argv[3]);  // min i j k, max i j k
  auto points = slurp<float>(argv[4]);
  auto samples = slurp<PFSample>(argv[5]);
  auto tf = slurp<double>(argv[6]);      // x y z, quaternion x y z w
  if (cells.size() != 6 || tf.size() != 7) { std::fprintf(stderr, "cells6 / tf7 sizes\n"); return 2; }
  const double res = std::atof(argv[7]), max_dist = std::atof(argv[8]);
  const int max_beams = std::atoi(argv[9]), gompertz = std::atoi(argv[10]);
  const int headings = std::atoi(argv[11]), stride = std::atoi(argv[12]), k = std::atoi(argv[13]);
  const long long cut1 = std::atoll(argv[14]), cut2 = std::atoll(argv[15]);

  auto eng = std::make_shared<Engine>(0);
  auto map = std::make_shared<OctoMap>(eng, res);
  map->setDistancesLUT(pose_indices, ratios, { cells[0], cells[1], cells[2] }, { cells[3], cells[4], cells[5] },
                       max_dist);

  // no ParticleFilter: the search and the seam need the map and a cloud model only
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

  int columns = 0;
  const long long total = scanner->searchSpace(headings, stride, &columns);
  if (!(0 < cut1 && cut1 < cut2 && cut2 < total)) { std::fprintf(stderr, "cuts outside the space of %lld\n", total); return 3; }
  dump(argv[16], scanner->searchPoses(data, headings, stride, k));
  std::vector<std::vector<bpf_pose_hit>> parts;
  parts.push_back(scanner->searchPoses(data, headings, stride, k, 0, cut1));
  parts.push_back(scanner->searchPoses(data, headings, stride, k, cut1, cut2 - cut1));
  parts.push_back(scanner->searchPoses(data, headings, stride, k, cut2));
  dump(argv[17], PointCloudScanner::mergePoseHits(parts, k));

  auto set = std::make_shared<PFSampleSet>();
  set->samples = samples;
  set->sample_count = (int)samples.size();
  const double sum = scanner->applyModelToSampleSet(data, set);
  dump(argv[18], set->samples);
  dump(argv[19], std::vector<double>{ sum });

  // the LUT back through the adapter: sizes only on stdout, the ratios to a file
  std::vector<uint32_t> pi_back;
  std::vector<uint8_t> dr_back;
  map->getDistancesLUT(&pi_back, &dr_back);
  dump(argv[20], dr_back);
  std::printf("%lld %d %zu %zu %zu %zu\n", total, columns, parts[0].size(), parts[1].size(), parts[2].size(),
              pi_back.size());
  return 0;
}
