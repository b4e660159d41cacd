// Stand-alone check of lvc_amd/csrc/patch_plan.h (tests/test_patch_plan_host.py builds it with the host compiler and
// -fsanitize=address,undefined and runs it).  No argument: every check below, exit status 0 / 1.  "plan direct|wino H W": prints the
// two-region plan of one map as  nreg tiles  then per region  y0 x0 h w PH PW tiles_y tiles_x.
//
// The single-shape choices are restated here from the kernels as they were before the planner (pick_patch_s of conv3x3_halo_s1.hip,
// the waste comparison of wino_launch), not taken from the header under test.
#include "patch_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <utility>
#include <vector>

static const int HM = 256, HALO_S1 = 340, MIN_PW = 4;
static int failures = 0;

#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      if (++failures <= 20) {                 \
        printf("FAIL %s: ", #cond);           \
        printf(__VA_ARGS__);                  \
        printf("\n");                         \
      }                                       \
    }                                         \
  } while (0)

static int cdiv(int a, int b) { return (a + b - 1) / b; }

// conv3x3_halo_s1.hip before the planner
static void old_pick_patch_s(int H, int W, int* PH, int* PW) {
  long long best_tiles = -1;
  int best_halo = 0, bh = 1, bw = 8;
  for (int pw = 4; pw <= 128; ++pw)
    for (int ph = 1; ph * pw <= HM; ++ph) {
      const int halo = (ph + 2) * (pw + 2);
      if (halo > HALO_S1) break;
      const long long tiles = (long long)cdiv(H, ph) * cdiv(W, pw);
      if (best_tiles < 0 || tiles < best_tiles || (tiles == best_tiles && halo < best_halo)) {
        best_tiles = tiles; best_halo = halo; bh = ph; bw = pw;
      }
    }
  *PH = bh; *PW = bw;
}

// conv3x3_wino.hip before the planner: (rows, pairs) -> here (rows, pixels)
static void old_wino_shape(int H, int W, int* PH, int* PW) {
  auto waste = [&](int phh, int pwp) { return (long long)cdiv(H, phh) * phh * cdiv(W, 2 * pwp) * 2 * pwp; };
  if (waste(16, 8) < waste(8, 16)) { *PH = 16; *PW = 16; } else { *PH = 8; *PW = 32; }
}

static bool shape_ok(bool wino, int PH, int PW) {
  if (wino) return (PH == 8 && PW == 32) || (PH == 16 && PW == 16);
  return PH >= 1 && PW >= MIN_PW && PH * PW <= HM && (PH + 2) * (PW + 2) <= HALO_S1;
}

static void check_map(LvcPatchPlanner& pl, bool wino, int H, int W, long long want_single, long long want_plan) {
  const char* kind = wino ? "wino" : "direct";
  const LvcPatchPlan one = pl.plan(H, W, false);
  const LvcPatchPlan two = pl.plan(H, W, true);
  int oph, opw;
  if (wino) old_wino_shape(H, W, &oph, &opw); else old_pick_patch_s(H, W, &oph, &opw);
  const long long old_tiles = (long long)cdiv(H, oph) * cdiv(W, opw);
  // the single-shape plan is what the kernels computed before
  CHECK(one.nreg == 1 && one.reg[0].PH == oph && one.reg[0].PW == opw && one.tiles == old_tiles, "%s %dx%d single %dx%d (%lld) old %dx%d (%lld)", kind, H, W,
        one.reg[0].PH, one.reg[0].PW, one.tiles, oph, opw, old_tiles);
  CHECK(one.reg[0].y0 == 0 && one.reg[0].x0 == 0 && one.reg[0].h == H && one.reg[0].w == W, "%s %dx%d single region", kind, H, W);
  // never more tiles; on a tie the single-shape plan itself
  CHECK(two.tiles <= one.tiles, "%s %dx%d plan %lld > single %lld", kind, H, W, two.tiles, one.tiles);
  if (two.tiles == one.tiles)
    CHECK(two.nreg == 1 && two.reg[0].PH == oph && two.reg[0].PW == opw, "%s %dx%d tie does not keep the single shape", kind, H, W);
  CHECK(two.nreg == 1 || two.nreg == 2, "%s %dx%d nreg %d", kind, H, W, two.nreg);
  // regions: constraints, counts, and an exact cover painted tile by tile (a tile is clipped to the map only: the region before the
  // split must end on a patch boundary by itself)
  std::vector<int> paint((size_t)H * W, 0);
  long long tiles = 0;
  for (int r = 0; r < two.nreg; ++r) {
    const LvcPatchRegion& g = two.reg[r];
    CHECK(shape_ok(wino, g.PH, g.PW), "%s %dx%d region %d shape %dx%d", kind, H, W, r, g.PH, g.PW);
    CHECK(g.h > 0 && g.w > 0 && g.y0 >= 0 && g.x0 >= 0 && g.y0 + g.h <= H && g.x0 + g.w <= W, "%s %dx%d region %d outside", kind, H, W, r);
    CHECK(g.tiles_y == cdiv(g.h, g.PH) && g.tiles_x == cdiv(g.w, g.PW), "%s %dx%d region %d tile counts", kind, H, W, r);
    if (wino) CHECK(g.x0 % 2 == 0, "%s %dx%d region %d starts at an odd column", kind, H, W, r);
    tiles += (long long)g.tiles_y * g.tiles_x;
    if (!shape_ok(wino, g.PH, g.PW)) continue;
    for (int ty = 0; ty < g.tiles_y; ++ty)
      for (int tx = 0; tx < g.tiles_x; ++tx)
        for (int py = 0; py < g.PH; ++py)
          for (int px = 0; px < g.PW; ++px) {
            const int y = g.y0 + ty * g.PH + py, x = g.x0 + tx * g.PW + px;
            if (y < H && x < W) ++paint[(size_t)y * W + x];
          }
  }
  CHECK(tiles == two.tiles, "%s %dx%d tiles %lld != sum %lld", kind, H, W, two.tiles, tiles);
  if (two.nreg == 2) {
    const LvcPatchRegion &a = two.reg[0], &b = two.reg[1];
    const bool rows = a.w == W && b.w == W && a.y0 == 0 && b.y0 == a.h && a.h + b.h == H && a.h % a.PH == 0 && a.x0 == 0 && b.x0 == 0;
    const bool cols = a.h == H && b.h == H && a.x0 == 0 && b.x0 == a.w && a.w + b.w == W && a.w % a.PW == 0 && a.y0 == 0 && b.y0 == 0;
    CHECK(rows || cols, "%s %dx%d split is neither whole patch rows nor whole patch columns", kind, H, W);
  }
  int bad = 0;
  for (size_t i = 0; i < paint.size(); ++i) bad += paint[i] != 1;
  CHECK(bad == 0, "%s %dx%d: %d pixels not covered exactly once", kind, H, W, bad);
  if (want_single >= 0) CHECK(one.tiles == want_single, "%s %dx%d single %lld want %lld", kind, H, W, one.tiles, want_single);
  if (want_plan >= 0) CHECK(two.tiles == want_plan, "%s %dx%d plan %lld want %lld", kind, H, W, two.tiles, want_plan);
  // memoised: the same answer again
  const LvcPatchPlan again = pl.plan(H, W, true);
  CHECK(memcmp(&again, &two, sizeof two) == 0, "%s %dx%d second look-up differs", kind, H, W);
}

// the fewest tiles any plan of the allowed form has, by exhaustive search written without the header's helpers
static long long brute(const std::vector<LvcPatchShape>& shapes, int H, int W) {
  static std::map<std::pair<size_t, std::pair<int, int>>, long long> memo;      // (shape list, h, w) -> fewest one-shape tiles
  auto single = [&](int h, int w) {
    const std::pair<size_t, std::pair<int, int>> key(shapes.size(), std::make_pair(h, w));
    auto it = memo.find(key);
    if (it != memo.end()) return it->second;
    long long b = -1;
    for (const LvcPatchShape& s : shapes) {
      const long long t = (long long)cdiv(h, s.PH) * cdiv(w, s.PW);
      if (b < 0 || t < b) b = t;
    }
    return memo[key] = b;
  };
  long long best = single(H, W);
  for (const LvcPatchShape& s : shapes) {
    for (int k = 1; k * s.PH < H; ++k) {
      const long long t = (long long)k * cdiv(W, s.PW) + single(H - k * s.PH, W);
      if (t < best) best = t;
    }
    for (int k = 1; k * s.PW < W; ++k) {
      const long long t = (long long)k * cdiv(H, s.PH) + single(H, W - k * s.PW);
      if (t < best) best = t;
    }
  }
  return best;
}

int main(int argc, char** argv) {
  LvcPatchPlanner direct = LvcPatchPlanner::direct(HM, HALO_S1, MIN_PW);
  LvcPatchPlanner wino = LvcPatchPlanner::winograd();
  if (argc == 5 && !strcmp(argv[1], "plan")) {
    const bool w = !strcmp(argv[2], "wino");
    const LvcPatchPlan p = (w ? wino : direct).plan(atoi(argv[3]), atoi(argv[4]), true);
    printf("%d %lld", p.nreg, p.tiles);
    for (int r = 0; r < p.nreg; ++r)
      printf("  %d %d %d %d %d %d %d %d", p.reg[r].y0, p.reg[r].x0, p.reg[r].h, p.reg[r].w, p.reg[r].PH, p.reg[r].PW, p.reg[r].tiles_y, p.reg[r].tiles_x);
    printf("\n");
    return 0;
  }
  for (const LvcPatchShape& s : direct.shapes()) CHECK(shape_ok(false, s.PH, s.PW), "direct shape %dx%d", s.PH, s.PW);
  for (int H = 1; H <= 64; ++H)
    for (int W = 1; W <= 64; ++W) {
      check_map(direct, false, H, W, -1, -1);
      check_map(wino, true, H, W, -1, -1);
    }
  // fewest tiles: against the exhaustive search on a grid of small maps and on the bench maps
  for (int H = 1; H <= 64; H += 3)
    for (int W = 1; W <= 64; W += 5) {
      CHECK(direct.plan(H, W, true).tiles == brute(direct.shapes(), H, W), "direct %dx%d not the fewest tiles", H, W);
      CHECK(wino.plan(H, W, true).tiles == brute(wino.shapes(), H, W), "wino %dx%d not the fewest tiles", H, W);
    }
  // the detector's maps at the bench shapes (tiles per image and channel tile)
  static const int rpn[5][3] = {{200, 336, 263}, {100, 168, 67}, {50, 84, 17}, {25, 42, 5}, {13, 21, 2}};
  int ph, pw;
  old_pick_patch_s(200, 336, &ph, &pw);                      // the grouped RPN launch: the largest map's shape on every level
  static const int rpn_now[5] = {272, 72, 20, 6, 2};
  long long now = 0, planned = 0;
  for (int l = 0; l < 5; ++l) {
    const int H = rpn[l][0], W = rpn[l][1];
    const long long t = (long long)cdiv(H, ph) * cdiv(W, pw);
    CHECK(t == rpn_now[l], "rpn level %d on the p2 shape %dx%d: %lld want %d", l, ph, pw, t, rpn_now[l]);
    now += t;
    // the issue's two-region counts came from hand-picked plans: an upper bound (100 x 168: 67 there, the search finds 66 --
    // 64 rows as 32 x 8, the other 36 as 18 x 14); what the planner must return is the exhaustive search's count, next line but one
    check_map(direct, false, H, W, -1, -1);
    CHECK(direct.plan(H, W, true).tiles <= rpn[l][2], "rpn level %d: %lld tiles, the table has %d", l, direct.plan(H, W, true).tiles, rpn[l][2]);
    planned += direct.plan(H, W, true).tiles;
    CHECK(direct.plan(H, W, true).tiles == brute(direct.shapes(), H, W), "direct %dx%d not the fewest tiles", H, W);
  }
  CHECK(now == 372 && planned == 353, "rpn head %lld -> %lld, want 372 -> 353 (the table's plans: 354)", now, planned);
  check_map(direct, false, 50, 84, 18, 17);                  // res4 conv2
  check_map(wino, true, 200, 336, 273, 263);                 // FPN output p2
  check_map(wino, true, 100, 168, 77, 72);                   // FPN output p3, res3 conv2
  CHECK(wino.plan(200, 336, true).tiles == brute(wino.shapes(), 200, 336), "wino p2 not the fewest tiles");
  CHECK(wino.plan(100, 168, true).tiles == brute(wino.shapes(), 100, 168), "wino p3 not the fewest tiles");
  if (failures) {
    printf("%d checks failed\n", failures);
    return 1;
  }
  printf("patch_plan: ok\n");
  return 0;
}
