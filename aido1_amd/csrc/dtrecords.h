// Internal: the checks of the record tables the handle is given -- the
// walkers and bots of the step (dt_set_*: double) and of the frame
// (dt_render_*: float), and dt_render_objects' records -- each written once.
// Plain C++: no HIP, nothing of the handle.  A check returns dt_last_error's
// text, empty for a table it accepts; `who` is the entry point's name.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dtsim.h"

namespace dtrec {

// What differs between the step's tables (dt_set_walkers, dt_set_bots) and
// the frame's (dt_render_walkers, dt_render_bots): the element type, the
// columns (a walker's K follows its W), and the words of the refusals.
struct Step {
  using T = double;
  static constexpr int kWalkStride = DT_WALK_STRIDE, kVel = 2, kW = 3, kBotStride = DT_OBJ_STRIDE;
  static constexpr const char *kWalkCount = "the handle's n_objects", *kBotCount = "n_objects",
                              *kBots = " is a bot's row (dt_set_bots)", *kRowArg = "object_row",
                              *kNoun = "row", *kOutside = "n_objects",
                              *kWalker = " is a walker's row (dt_set_walkers)";
};
struct Frame {
  using T = float;
  static constexpr int kWalkStride = DT_RENDER_WALK_STRIDE, kVel = -1, kW = 2,
                       kBotStride = DT_RENDER_OBJ_STRIDE;
  static constexpr const char *kWalkCount = "the count dt_render_objects was given",
                              *kBotCount = kWalkCount,
                              *kBots = " is a render bot's record (dt_render_bots)",
                              *kRowArg = "render_row", *kNoun = "record",
                              *kOutside = "dt_render_objects' count",
                              *kWalker = " is a render walker's";
};

// dt_set_walkers' packed row, as the kernels read it (dt::kWalkRec doubles):
// home x, z, vel, then the word W | K << 32 (K = 0: a static object).
constexpr int kWalkPacked = 4;

inline bool packed_walks(const std::vector<double>& packed, int32_t o) {
  if (packed.empty()) return false;
  uint64_t wk;
  memcpy(&wk, packed.data() + (size_t)o * kWalkPacked + 3, 8);
  return (uint32_t)(wk >> 32) != 0u;
}

template <class T>
const T* nonfinite(const T* v, size_t count) {   // the first, or v + count
  return std::find_if_not(v, v + count, [](T x) { return std::isfinite(x); });
}

// a table of `count` elements, `per` of them to the `noun` the text names
template <class T>
std::string finite(const std::string& who, const char* noun, const T* v, size_t count,
                   size_t per) {
  const T* bad = nonfinite(v, count);
  if (bad == v + count) return "";
  return who + ": " + noun + " " + std::to_string((size_t)(bad - v) / per) +
         " holds a non-finite value";
}

inline std::string objects(const std::string& who, const float* recs, int32_t n) {
  if (n < 0 || n > DT_MAX_RENDER_OBJECTS)
    return who + ": n must be in 0.." + std::to_string(DT_MAX_RENDER_OBJECTS);
  if (n > 0 && !recs) return who + ": recs is null";
  return finite(who, "record", recs, (size_t)n * DT_RENDER_OBJ_STRIDE, DT_RENDER_OBJ_STRIDE);
}

// a walker value that must be a whole number of steps in [0, 2^24)
template <class T>
bool whole_steps(T v) {
  return v >= 0 && v < 16777216 && v == std::floor(v);
}

// A row per record, `count` of them or none; the `n_bots` rows of `bot_row`
// may not walk.  `packed` (the step's rows only) receives the packed rows.
template <class L>
std::string walkers(const std::string& who, const typename L::T* recs, int32_t n, int32_t count,
                    const int32_t* bot_row, size_t n_bots, std::vector<double>* packed = nullptr) {
  using T = typename L::T;
  if (n != 0 && n != count)
    return who + ": n must be 0 or " + L::kWalkCount + " (" + std::to_string(count) + ")";
  if (n > 0 && !recs) return who + ": recs is null";
  if (packed) packed->assign((size_t)n * kWalkPacked, 0.0);
  for (int32_t o = 0; o < n; ++o) {
    const T* r = recs + (size_t)o * L::kWalkStride;
    const std::string row = who + ": row " + std::to_string(o);
    if (nonfinite(r, L::kWalkStride) != r + L::kWalkStride) return row + " holds a non-finite value";
    if (std::all_of(r, r + L::kWalkStride, [](T v) { return v == 0; })) continue;   // a static object
    if constexpr (L::kVel >= 0)
      if (!(r[L::kVel] > 0)) return row + ": vel must be > 0";
    const T W = r[L::kW], K = r[L::kW + 1];
    if (!whole_steps(W) || !whole_steps(K))
      return row + ": W and K must be whole numbers in [0, 2^24)";
    if (K < 1) return row + ": K must be >= 1";
    if (std::find(bot_row, bot_row + n_bots, o) != bot_row + n_bots) return row + L::kBots;
    if constexpr (L::kVel >= 0)
      if (packed) {
        double* d = packed->data() + (size_t)o * kWalkPacked;
        d[0] = r[0], d[1] = r[1], d[2] = r[L::kVel];
        const uint64_t wk = (uint64_t)(uint32_t)W | ((uint64_t)(uint32_t)K << 32);
        memcpy(d + 3, &wk, 8);
      }
  }
  return "";
}

// `rows` rows of `n` bot records, bot b standing for record row[b] of `count`;
// is_walker(o): record o walks, so no bot may name it.  `col` receives each
// record's bot or -1 (DT_MAX_RENDER_OBJECTS entries at least).
template <class L, class IsWalker>
std::string bots(const std::string& who, const typename L::T* recs, const int32_t* row,
                 int32_t rows, int32_t n, int32_t count, IsWalker is_walker,
                 std::vector<int32_t>& col) {
  if (n < 0 || n > count)
    return who + ": n must be in 0.." + L::kBotCount + " (" + std::to_string(count) + ")";
  col.assign((size_t)std::max(count, DT_MAX_RENDER_OBJECTS), -1);
  if (n == 0) return "";
  if (!recs || !row) return who + ": recs and " + L::kRowArg + " are required";
  if (rows < 1 || rows > DT_MAX_BOT_ROWS)
    return who + ": rows must be in 1.." + std::to_string(DT_MAX_BOT_ROWS);
  const size_t cnt = (size_t)rows * n * L::kBotStride, bytes = cnt * sizeof(typename L::T);
  if (bytes > (size_t)DT_MAX_BOT_BYTES)
    return who + ": the table (" + std::to_string(bytes) + " B) is over " +
           std::to_string(DT_MAX_BOT_BYTES) + " B";
  for (int32_t b = 0; b < n; ++b) {
    const int32_t o = row[b];
    const std::string bot =
        who + ": bot " + std::to_string(b) + ": " + L::kNoun + " " + std::to_string(o);
    if (o < 0 || o >= count) return bot + " is outside " + L::kOutside;
    if (col[o] >= 0) return bot + " is named twice";
    if (is_walker(o)) return bot + L::kWalker;
    col[o] = b;
  }
  return finite(who, "row", recs, cnt, (size_t)n * L::kBotStride);
}

}  // namespace dtrec
