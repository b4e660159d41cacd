// patch_plan.h -- host-only planner of the 3x3 kernels' pixel patches (conv3x3_halo_s1.hip, conv3x3_wino.hip).  No HIP in here: the
// unit test builds it with the host compiler (tests/native/patch_plan_main.cpp).
//
// Both kernels pay a full 256-pixel MFMA tile for every patch, whatever its fill, and used ONE patch shape per map.  A map whose
// height (or width) is no multiple of the best shape's wastes up to a patch row (column) of tiles on the overhang: 200 x 336 as
// 16 x 16 patches = 13 x 21 = 273 tiles for 262.5 tiles' worth of pixels.  The planner returns AT MOST TWO regions per map, split
// after a whole number of patch rows or of patch columns of the first region's shape, each with its own shape: the first 8 rows as
// 8 x 32 (11 tiles) + the other 192 as 16 x 16 (252) = 263.  Region 0 is exact along the split axis, so the kernels' existing "pixel
// inside the map" masks are all the clipping a tile needs; the convolution's halo is read from the whole map, not from the region.
//
// Rules: fewest tiles; on a tie the single-shape plan wins, and that shape is the one the kernels picked before the planner existed
// (fewest tiles, then the smaller rank -- the halo for the direct kernel, none for Winograd -- then the first in list order);
// among two-region plans of equal count the smaller sum of tiles x rank, then the first found.  Plans and single-shape answers are
// memoised per planner (= per kernel and constraint set) and map size: a launch costs one map look-up.
#pragma once
#include <map>
#include <utility>
#include <vector>

struct LvcPatchRegion {
  int y0, x0, h, w;          // the region's pixels: rows [y0, y0 + h), columns [x0, x0 + w)
  int PH, PW;                // patch shape in pixels
  int tiles_y, tiles_x;      // ceil(h / PH), ceil(w / PW)
};
struct LvcPatchPlan {
  int nreg;                  // 1 or 2
  long long tiles;           // per image and channel tile
  LvcPatchRegion reg[2];
};
struct LvcPatchShape {
  int PH, PW, rank;
};

class LvcPatchPlanner {
 public:
  // direct kernel: PH PW <= max_area, (PH + 2)(PW + 2) <= max_halo, PW >= min_pw; rank = the halo (its staging cost)
  static LvcPatchPlanner direct(int max_area, int max_halo, int min_pw) {
    LvcPatchPlanner p;
    for (int pw = min_pw; pw <= max_area; ++pw)
      for (int ph = 1; ph * pw <= max_area; ++ph) {
        const int halo = (ph + 2) * (pw + 2);
        if (halo > max_halo) break;
        p.shapes_.push_back({ph, pw, halo});
      }
    return p;
  }
  // Winograd: the two shapes its V buffer is laid out for -- 8 rows x 16 pairs first (it wins a tie), 16 rows x 8 pairs
  static LvcPatchPlanner winograd() {
    LvcPatchPlanner p;
    p.shapes_.push_back({8, 32, 0});
    p.shapes_.push_back({16, 16, 0});
    return p;
  }
  const std::vector<LvcPatchShape>& shapes() const { return shapes_; }

  // the one-shape decomposition of an h x w map
  LvcPatchShape single(int h, int w) {
    const std::pair<int, int> key(h, w);
    auto it = singles_.find(key);
    if (it != singles_.end()) return it->second;
    long long best = -1;
    LvcPatchShape bs = shapes_[0];
    for (const LvcPatchShape& s : shapes_) {
      const long long t = count(h, w, s);
      if (best < 0 || t < best || (t == best && s.rank < bs.rank)) { best = t; bs = s; }
    }
    singles_[key] = bs;
    return bs;
  }
  static long long count(int h, int w, const LvcPatchShape& s) { return (long long)cdiv(h, s.PH) * cdiv(w, s.PW); }

  // two_regions = false: the single-shape plan
  const LvcPatchPlan& plan(int H, int W, bool two_regions) {
    const std::pair<int, int> key(H, W);
    std::map<std::pair<int, int>, LvcPatchPlan>& memo = two_regions ? plans2_ : plans1_;
    auto it = memo.find(key);
    if (it != memo.end()) return it->second;
    LvcPatchPlan best;
    best.nreg = 1;
    best.reg[0] = region(0, 0, H, W, single(H, W));
    best.reg[1] = best.reg[0];
    best.tiles = tiles_of(best.reg[0]);
    if (two_regions) {
      long long best_cost = -1;
      auto consider = [&](const LvcPatchRegion& a, const LvcPatchShape& sa, const LvcPatchRegion& b, const LvcPatchShape& sb) {
        const long long t = tiles_of(a) + tiles_of(b);
        const long long cost = tiles_of(a) * sa.rank + tiles_of(b) * sb.rank;
        if (t < best.tiles || (best.nreg == 2 && t == best.tiles && cost < best_cost)) {
          best.nreg = 2; best.tiles = t; best.reg[0] = a; best.reg[1] = b; best_cost = cost;
        }
      };
      // the one-shape answers for what a split leaves over, looked up once per size
      std::vector<LvcPatchShape> below(H), right(W);
      for (int h = 1; h < H; ++h) below[h] = single(h, W);
      for (int w = 1; w < W; ++w) right[w] = single(H, w);
      for (const LvcPatchShape& s : shapes_) {
        for (int rows = s.PH; rows < H; rows += s.PH)          // split after whole patch rows
          consider(region(0, 0, rows, W, s), s, region(rows, 0, H - rows, W, below[H - rows]), below[H - rows]);
        for (int cols = s.PW; cols < W; cols += s.PW)          // ... or after whole patch columns
          consider(region(0, 0, H, cols, s), s, region(0, cols, H, W - cols, right[W - cols]), right[W - cols]);
      }
    }
    return memo[key] = best;
  }

 private:
  static int cdiv(int a, int b) { return (a + b - 1) / b; }
  static long long tiles_of(const LvcPatchRegion& r) { return (long long)r.tiles_y * r.tiles_x; }
  static LvcPatchRegion region(int y0, int x0, int h, int w, const LvcPatchShape& s) {
    return LvcPatchRegion{y0, x0, h, w, s.PH, s.PW, cdiv(h, s.PH), cdiv(w, s.PW)};
  }
  std::vector<LvcPatchShape> shapes_;
  std::map<std::pair<int, int>, LvcPatchShape> singles_;
  std::map<std::pair<int, int>, LvcPatchPlan> plans1_, plans2_;
};
