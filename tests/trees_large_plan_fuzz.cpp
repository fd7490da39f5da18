// Stand-alone program over miosqp_amd/csrc/trees_large_plan.hpp (built with -fsanitize=address,undefined by
// tests/test_solve_many_large_cpu.py and run as a subprocess): the layout of the arena of miosqp_qp_solve_trees_large on
// a few thousand random (n, M, p, B, leaf_cap) against a straightforward restatement of the sizes -- every array inside
// the arena, no two arrays overlapping, the staged part in front, what comes back at its end --, and B and leaf_cap near
// overflow refused instead of wrapped.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "../miosqp_amd/csrc/trees_large_plan.hpp"

namespace tl = miosqp::trees_large;

static int fails = 0;
#define EXPECT(c)                                 \
  do {                                            \
    if (!(c)) {                                   \
      std::printf("line %d: %s\n", __LINE__, #c); \
      fails++;                                    \
    }                                             \
  } while (0)

// the doubles the issue counts per instance, restated without the header: leaf_cap x (2 p + n + M) of leaf store, the
// staging block (3 M + n), q raw and scaled (2 n), the incumbent and its value (n + 1), the outcome (6); rf: 4 counters;
// sb: 4 counters, the work area and leaf_cap x 4 of Node.pc
static unsigned __int128 per_instance(unsigned __int128 n, unsigned __int128 M, unsigned __int128 p, unsigned __int128 cap, int v) {
  unsigned __int128 d = cap * (2 * p + n + M) + (3 * M + n) + 2 * n + (n + 1) + 6;
  if (v == tl::RF) d += 4;
  if (v == tl::SB) d += 4 + miosqp::tree_sb::work_doubles((int)p) + cap * 4;
  return d;
}

static void layouts() {
  std::mt19937 rng(20261021);
  size_t filled = 0;
  for (int trial = 0; trial < 4000; trial++) {
    const int n = 1 + (int)(rng() % 200), p = 1 + (int)(rng() % n), M = p + (int)(rng() % 600);
    const int B = 1 + (int)(rng() % (trial % 8 == 0 ? 4000 : 40)), cap = 2 + (int)(rng() % (trial % 8 == 0 ? 1100 : 40));
    const tl::Variant v = (tl::Variant)(rng() % 3);
    tl::Plan P;
    std::string err;
    EXPECT(tl::plan(n, M, p, B, cap, v, P, err) == 0);
    const size_t sn = n, sM = M, sp = p, sB = B, sc = cap;
    std::vector<std::pair<size_t, size_t>> iv;  // [begin, end) of every array
    iv.push_back({P.raw, P.raw + sB * (3 * sM + sn)});
    iv.push_back({P.qraw, P.qraw + sB * sn});
    iv.push_back({P.upper, P.upper + sB});
    iv.push_back({P.inc, P.inc + sB * sn});
    iv.push_back({P.out, P.out + sB * tl::OUT_DOUBLES});
    if (v == tl::RF) iv.push_back({P.rf, P.rf + sB * tl::RF_DOUBLES});
    if (v == tl::SB) iv.push_back({P.sb, P.sb + sB * tl::SB_DOUBLES});
    iv.push_back({P.q, P.q + sB * sn});
    iv.push_back({P.lf_lo, P.lf_lo + sB * sc * sp});
    iv.push_back({P.lf_hi, P.lf_hi + sB * sc * sp});
    iv.push_back({P.lf_x, P.lf_x + sB * sc * sn});
    iv.push_back({P.lf_y, P.lf_y + sB * sc * sM});
    if (v == tl::SB) {
      iv.push_back({P.sb_work, P.sb_work + sB * miosqp::tree_sb::work_doubles(p)});
      iv.push_back({P.sb_pc, P.sb_pc + sB * sc * (size_t)miosqp::tree_sb::PC_DOUBLES});
    }
    // the sizes: the restatement, and nothing but alignment beyond it (16 bytes per array, 256 bytes behind the upload)
    const unsigned __int128 want = (unsigned __int128)B * per_instance(n, M, p, cap, v);
    EXPECT((unsigned __int128)P.total_doubles >= want && (unsigned __int128)P.total_doubles <= want + 14 + 32);
    size_t sum = 0;
    for (const auto &a : iv) sum += a.second - a.first;
    EXPECT((unsigned __int128)sum == want);
    // staged: raw, qraw, upper in front of what comes back; inc, out and the records inside it; the rest behind the upload
    EXPECT(P.down_off + P.down_doubles == P.up_doubles && P.up_doubles <= P.total_doubles);
    EXPECT(P.upper + sB <= P.down_off && P.inc == P.down_off);
    EXPECT(P.q >= P.up_doubles && P.q % 32 == 0);
    for (size_t k = 0; k < iv.size(); k++) EXPECT(iv[k].first % 2 == 0);  // 16-byte starts
    EXPECT(std::max({P.out + sB * tl::OUT_DOUBLES, P.rf + (v == tl::RF ? sB * tl::RF_DOUBLES : 0),
                     P.sb + (v == tl::SB ? sB * tl::SB_DOUBLES : 0)}) <= P.up_doubles);
    // adjacent arrays do not overlap, all inside the arena
    std::sort(iv.begin(), iv.end());
    for (size_t k = 0; k < iv.size(); k++) {
      EXPECT(iv[k].first < iv[k].second && iv[k].second <= P.total_doubles);
      if (k) EXPECT(iv[k - 1].second <= iv[k].first);
    }
    // instance b of an array lies at b x (its size): the last instance ends where the array ends (what the kernel's
    // tree_instance forms: b * cap * p and so on, in size_t)
    EXPECT(P.lf_y + (sB - 1) * sc * sM + sc * sM == P.lf_y + sB * sc * sM);
    // the plan is what the host and the kernel write through: fill every array of a real buffer, where it is small
    // enough (the sanitizer watches the ends)
    if (P.total_doubles <= ((size_t)1 << 21) && filled < ((size_t)1 << 27)) {
      filled += P.total_doubles;
      std::vector<unsigned char> arena(P.total_doubles, 0);
      for (const auto &a : iv)
        for (size_t i = a.first; i < a.second; i++) arena[i]++;
      size_t twice = 0;
      for (unsigned char c : arena) twice += c > 1;
      EXPECT(twice == 0);
    }
    // the room check: the arena itself is enough, one double less is not, and the text names B and the bytes
    EXPECT(tl::check_room(P, B, P.total_doubles, err) == 0);
    EXPECT(tl::check_room(P, B, P.total_doubles - 1, err) == tl::ERR_ARG);
    EXPECT(err.find("B = " + std::to_string(B)) != std::string::npos &&
           err.find(std::to_string(P.total_doubles * sizeof(double)) + " bytes") != std::string::npos);
  }
}

static void refusals() {
  tl::Plan P;
  std::string err;
  const int big = std::numeric_limits<int32_t>::max();
  // arguments below their minimum
  EXPECT(tl::plan(10, 20, 3, 0, 256, tl::PLAIN, P, err) == tl::ERR_ARG);
  EXPECT(tl::plan(10, 20, 3, 4, 1, tl::PLAIN, P, err) == tl::ERR_ARG);
  EXPECT(tl::plan(0, 20, 3, 4, 256, tl::PLAIN, P, err) == tl::ERR_ARG);
  // B x leaf_cap x M at the largest values an int32 holds: 2^31 x 2^31 x 2^11 doubles does not fit 64 bits
  for (int v = 0; v < 3; v++) {
    err.clear();
    EXPECT(tl::plan(200, 2048, 100, big, big, (tl::Variant)v, P, err) == tl::ERR_ARG);
    EXPECT(err.find("B = " + std::to_string(big)) != std::string::npos && err.find("leaf_cap " + std::to_string(big)) != std::string::npos);
    EXPECT(P.total_doubles == 0);
  }
  // the largest shapes whose doubles still fit 64 bits but whose BYTES do not: refused as well
  // (2^31 - 1) x (2^31 - 1) x 1 doubles is below 2^62; with M = 2 the y store alone is 2^63 doubles = 2^66 bytes
  EXPECT(tl::plan(1, 2, 1, big, big, tl::PLAIN, P, err) == tl::ERR_ARG);
  // ... and near the edge from below: sizes that fit are planned, exactly
  {
    const int B = 1 << 20, cap = 1 << 20;  // 2^40 x (2 + 1 + 1) doubles of leaf store: 2^45 bytes
    EXPECT(tl::plan(1, 1, 1, B, cap, tl::SB, P, err) == 0);
    const unsigned __int128 want = (unsigned __int128)B * per_instance(1, 1, 1, cap, tl::SB);
    EXPECT((unsigned __int128)P.total_doubles >= want && (unsigned __int128)P.total_doubles <= want + 46);
    EXPECT(tl::check_room(P, B, (size_t)1 << 30, err) == tl::ERR_ARG);
  }
  // walk leaf_cap up at the largest B: every answer is either a refusal or a plan that holds the restated size
  for (int sh = 1; sh <= 31; sh++) {
    const int cap = (int)std::min<int64_t>(((int64_t)1 << sh), big);
    const int rc = tl::plan(197, 1851, 197, big, cap, tl::SB, P, err);
    const unsigned __int128 want = (unsigned __int128)big * per_instance(197, 1851, 197, cap, tl::SB);
    if (rc == 0) EXPECT((unsigned __int128)P.total_doubles >= want);
    else EXPECT(rc == tl::ERR_ARG && (want + 46) * 8 + 4096 > (unsigned __int128)std::numeric_limits<size_t>::max());
  }
}

int main() {
  layouts();
  refusals();
  if (fails) {
    std::printf("%d failures\n", fails);
    return 1;
  }
  std::printf("trees_large_plan ok\n");
  return 0;
}
