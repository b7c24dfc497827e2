// Host-only check of csrc/dtrecords.h (the record tables' refusals, whole
// texts) and csrc/dtdevbuf.h (the handle's two upload rules), built with
// AddressSanitizer + UBSan by tests/test_host_tables.py.  No HIP library is
// linked: the five HIP calls the headers make are the stand-ins below, which
// keep "device" memory on the heap (so an upload past a capacity is a heap
// overflow the sanitizer reports, and a dropped allocation a leak), count the
// live allocations, log allocations and frees, and fail the k-th call on
// request.  Exit status 0: every check held.
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "../aido1_amd/csrc/dtdevbuf.h"
#include "../aido1_amd/csrc/dtrecords.h"

static int g_live = 0, g_calls = 0, g_fail_at = 0;   // g_fail_at: 0 never
static std::string g_log;                            // 'm' hipMalloc, 'f' hipFree, 's' sync

static bool injected() { return ++g_calls == g_fail_at; }

extern "C" {
hipError_t hipMalloc(void** ptr, size_t size) {
  if (injected()) return hipErrorOutOfMemory;
  *ptr = malloc(size ? size : 1);
  ++g_live;
  g_log += 'm';
  return hipSuccess;
}
hipError_t hipFree(void* ptr) {
  if (ptr) --g_live, g_log += 'f';
  free(ptr);
  return hipSuccess;
}
hipError_t hipMemcpy(void* dst, const void* src, size_t n, hipMemcpyKind) {
  if (injected()) return hipErrorUnknown;
  memcpy(dst, src, n);
  return hipSuccess;
}
hipError_t hipDeviceSynchronize(void) {
  if (injected()) return hipErrorUnknown;
  g_log += 's';
  return hipSuccess;
}
const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "injected"; }
}

static int g_bad = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #c); \
      ++g_bad;                                                    \
    }                                                             \
  } while (0)
#define SAME(got, want) same(__LINE__, (got), (want))
static void same(int line, const std::string& got, const std::string& want) {
  if (got == want) return;
  fprintf(stderr, "line %d: got  \"%s\"\n         want \"%s\"\n", line, got.c_str(), want.c_str());
  ++g_bad;
}

using namespace dtrec;
static const double kNaN = std::numeric_limits<double>::quiet_NaN();
static const double kInf = std::numeric_limits<double>::infinity();
static const int kMax = DT_MAX_RENDER_OBJECTS;
static const double kTop = 16777215.0;   // 2^24 - 1

// ---- dt_render_objects ----------------------------------------------------
static void objects_cases() {
  const char* who = "dt_render_objects";
  std::vector<float> r((size_t)kMax * DT_RENDER_OBJ_STRIDE, 1.0f);
  SAME(objects(who, nullptr, 0), "");
  SAME(objects(who, r.data(), 1), "");
  SAME(objects(who, r.data(), kMax), "");
  SAME(objects(who, r.data(), -1), "dt_render_objects: n must be in 0..256");
  SAME(objects(who, r.data(), kMax + 1), "dt_render_objects: n must be in 0..256");
  SAME(objects(who, nullptr, 1), "dt_render_objects: recs is null");
  SAME(objects(who, nullptr, kMax + 1), "dt_render_objects: n must be in 0..256");   // two faults
  r.front() = (float)kNaN;
  SAME(objects(who, r.data(), kMax), "dt_render_objects: record 0 holds a non-finite value");
  r.front() = 1.0f, r.back() = (float)kInf;
  SAME(objects(who, r.data(), kMax), "dt_render_objects: record 255 holds a non-finite value");
  SAME(objects(who, r.data(), kMax - 1), "");
  r[DT_RENDER_OBJ_STRIDE] = (float)-kInf;   // two faults: the first record in the table is named
  SAME(objects(who, r.data(), kMax), "dt_render_objects: record 1 holds a non-finite value");
}

// ---- dt_set_walkers / dt_render_walkers -----------------------------------
// One body for both layouts: `who`, the words in kWalkCount / kBots and the
// columns are what differ.  A row is built as (a, b, [vel], W, K).
template <class L>
static std::vector<typename L::T> walk_table(int n, double W, double K) {
  std::vector<typename L::T> t((size_t)n * L::kWalkStride);
  for (int o = 0; o < n; ++o) {
    typename L::T* r = t.data() + (size_t)o * L::kWalkStride;
    r[0] = 0.5f, r[1] = -0.25f;
    if (L::kVel >= 0) r[L::kVel] = 0.125f;
    r[L::kW] = (typename L::T)W, r[L::kW + 1] = (typename L::T)K;
  }
  return t;
}

template <class L>
static void walker_cases(const std::string& who, const std::string& count_words,
                         const std::string& bots_words) {
  using T = typename L::T;
  const int32_t none = 0;
  auto run = [&](const std::vector<T>& t, int n, int count, std::vector<int32_t> bots = {}) {
    return walkers<L>(who, t.data(), n, count, bots.empty() ? &none : bots.data(), bots.size());
  };
  const std::string row0 = who + ": row 0", steps = ": W and K must be whole numbers in [0, 2^24)";
  SAME(walkers<L>(who, nullptr, 0, 3, &none, 0), "");
  SAME(run(walk_table<L>(1, 3, 2), 1, 1), "");
  SAME(run(walk_table<L>(kMax, 3, 2), kMax, kMax), "");
  SAME(run(walk_table<L>(2, 3, 2), 2, 3), who + ": n must be 0 or " + count_words + " (3)");
  SAME(run(walk_table<L>(1, 3, 2), -1, 3), who + ": n must be 0 or " + count_words + " (3)");
  SAME(walkers<L>(who, nullptr, 3, 3, &none, 0), who + ": recs is null");
  SAME(walkers<L>(who, nullptr, 2, 3, &none, 0),   // two faults: the count first
       who + ": n must be 0 or " + count_words + " (3)");
  auto t = walk_table<L>(kMax, 3, 2);
  t.front() = (T)kNaN;
  SAME(run(t, kMax, kMax), row0 + " holds a non-finite value");
  t = walk_table<L>(kMax, 3, 2);
  t.back() = (T)kInf;
  SAME(run(t, kMax, kMax), who + ": row 255 holds a non-finite value");
  SAME(run(walk_table<L>(1, kTop, 2), 1, 1), "");
  SAME(run(walk_table<L>(1, 3, kTop), 1, 1), "");
  SAME(run(walk_table<L>(1, kTop + 1, 2), 1, 1), row0 + steps);
  SAME(run(walk_table<L>(1, 3, kTop + 1), 1, 1), row0 + steps);
  SAME(run(walk_table<L>(1, 2.5, 2), 1, 1), row0 + steps);
  SAME(run(walk_table<L>(1, -1, 2), 1, 1), row0 + steps);
  SAME(run(walk_table<L>(1, 3, 0), 1, 1), row0 + ": K must be >= 1");
  SAME(run(std::vector<T>(L::kWalkStride, (T)0), 1, 1), "");   // all zero: a static object
  SAME(run(walk_table<L>(1, 2.5, 0), 1, 1), row0 + steps);   // two faults: W before K
  // a bot's row may not walk; it may stand (all zero); rows of bots switched off do not count
  SAME(run(walk_table<L>(3, 3, 2), 3, 3, {1}), who + ": row 1" + bots_words);
  SAME(run(walk_table<L>(3, 3, 2), 3, 3, {2, 0}), who + ": row 0" + bots_words);
  SAME(walkers<L>(who, walk_table<L>(3, 3, 2).data(), 3, 3, &none, 0), "");
  t = walk_table<L>(3, 3, 2);
  std::fill(t.begin() + L::kWalkStride, t.begin() + 2 * L::kWalkStride, (T)0);
  SAME(run(t, 3, 3, {1}), "");
  SAME(run(walk_table<L>(3, 3, 0), 3, 3, {0}), row0 + ": K must be >= 1");   // two faults
  t = walk_table<L>(3, 3, 2);   // two faults: row 0's comes before row 1's NaN
  t[L::kW] = (T)0.5, t[L::kWalkStride] = (T)kNaN;
  SAME(run(t, 3, 3), row0 + steps);
}

static void step_walker_cases() {
  const char* who = "dt_set_walkers";
  const int32_t none = 0;
  auto t = walk_table<Step>(1, 3, 2);
  t[2] = 0.0;
  SAME(walkers<Step>(who, t.data(), 1, 1, &none, 0), "dt_set_walkers: row 0: vel must be > 0");
  t[2] = -1.0, t[3] = 2.5;   // two faults: vel before W
  SAME(walkers<Step>(who, t.data(), 1, 1, &none, 0), "dt_set_walkers: row 0: vel must be > 0");
  // the packed rows: home, vel and W | K << 32; a static row stays zero; n = 0: none
  t = walk_table<Step>(2, kTop, 7);
  std::fill(t.begin(), t.begin() + DT_WALK_STRIDE, 0.0);
  std::vector<double> packed(5, 1.0);
  SAME(walkers<Step>(who, t.data(), 2, 2, &none, 0, &packed), "");
  CHECK(packed.size() == 2 * (size_t)kWalkPacked);
  uint64_t wk[2];
  memcpy(&wk[0], &packed[3], 8), memcpy(&wk[1], &packed[kWalkPacked + 3], 8);
  CHECK(packed[0] == 0.0 && packed[1] == 0.0 && packed[2] == 0.0 && wk[0] == 0);
  CHECK(packed[4] == 0.5 && packed[5] == -0.25 && packed[6] == 0.125);
  CHECK(wk[1] == (16777215ull | 7ull << 32));
  CHECK(!packed_walks(packed, 0) && packed_walks(packed, 1));
  SAME(walkers<Step>(who, nullptr, 0, 2, &none, 0, &packed), "");
  CHECK(packed.empty() && !packed_walks(packed, 1));
}

// ---- dt_set_bots / dt_render_bots -----------------------------------------
template <class L>
static void bot_cases(const std::string& who, const std::string& count_words,
                      const std::string& row_arg, const std::string& noun,
                      const std::string& outside, const std::string& walker_words) {
  using T = typename L::T;
  std::vector<int32_t> col;
  int walker = -1;   // the record that walks
  auto walks = [&](int32_t o) { return o == walker; };
  auto run = [&](const std::vector<T>& t, std::vector<int32_t> row, int rows, int count) {
    return bots<L>(who, t.data(), row.data(), rows, (int32_t)row.size(), count, walks, col);
  };
  auto table = [](size_t rows, size_t n) { return std::vector<T>(rows * n * L::kBotStride, (T)1); };
  std::vector<int32_t> all(kMax);
  for (int i = 0; i < kMax; ++i) all[i] = kMax - 1 - i;
  const std::string range = who + ": n must be in 0.." + count_words;
  const std::string rows_text = who + ": rows must be in 1.." + std::to_string(DT_MAX_BOT_ROWS);

  SAME(bots<L>(who, nullptr, nullptr, 0, 0, 3, walks, col), "");
  SAME(run(table(1, 1), {2}, 1, 3), "");
  CHECK(col.size() == (size_t)kMax && col[2] == 0 && col[0] == -1 && col[1] == -1 && col[3] == -1);
  SAME(run(table(1, kMax), all, 1, kMax), "");
  CHECK(col[0] == kMax - 1 && col[kMax - 1] == 0);
  SAME(run(table(DT_MAX_BOT_ROWS, 1), {0}, DT_MAX_BOT_ROWS, 1), "");
  SAME(bots<L>(who, nullptr, nullptr, 1, -1, 3, walks, col), range + " (3)");
  SAME(run(table(1, 4), {0, 1, 2, 3}, 1, 3), range + " (3)");
  SAME(bots<L>(who, nullptr, nullptr, 0, 4, 3, walks, col), range + " (3)");   // two faults
  const std::vector<T> one = table(1, 1);
  const int32_t r0 = 0;
  SAME(bots<L>(who, nullptr, &r0, 1, 1, 3, walks, col), who + ": recs and " + row_arg + " are required");
  SAME(bots<L>(who, one.data(), nullptr, 1, 1, 3, walks, col),
       who + ": recs and " + row_arg + " are required");
  SAME(bots<L>(who, nullptr, nullptr, 0, 1, 3, walks, col),   // two faults: the pointers first
       who + ": recs and " + row_arg + " are required");
  SAME(run(one, {0}, 0, 3), rows_text);
  SAME(run(one, {0}, DT_MAX_BOT_ROWS + 1, 3), rows_text);
  SAME(run(one, {7}, 0, 3), rows_text);   // two faults: rows before the row indices
  {
    // the byte cap: the largest table of 128 bots under it is accepted (for
    // the frame's 32-byte records that is the cap exactly; the step's
    // 160-byte records do not divide it), one row more is refused -- before
    // the table is read, so the refused call gets by with a short one
    const size_t n = 128, rec = L::kBotStride * sizeof(T), rows = DT_MAX_BOT_BYTES / (n * rec);
    CHECK(sizeof(T) != 4 || rows * n * rec == (size_t)DT_MAX_BOT_BYTES);
    const std::vector<int32_t> row(all.begin(), all.begin() + n);
    SAME(run(table(rows, n), row, (int)rows, kMax), "");
    SAME(run(one, row, (int)rows + 1, kMax),
         who + ": the table (" + std::to_string((rows + 1) * n * rec) + " B) is over 268435456 B");
  }
  SAME(run(one, {-1}, 1, 3), who + ": bot 0: " + noun + " -1 is outside " + outside);
  SAME(run(one, {3}, 1, 3), who + ": bot 0: " + noun + " 3 is outside " + outside);
  SAME(run(table(2, 3), {1, 1, 2}, 2, 3), who + ": bot 1: " + noun + " 1 is named twice");
  SAME(run(table(2, 3), {0, 2, 2}, 2, 3), who + ": bot 2: " + noun + " 2 is named twice");
  walker = 1;
  SAME(run(table(2, 2), {0, 1}, 2, 3), who + ": bot 1: " + noun + " 1" + walker_words);
  SAME(run(table(2, 2), {0, 2}, 2, 3), "");
  SAME(run(table(2, 3), {0, 1, 1}, 2, 3),   // two faults: bot 1 is a walker's before bot 2 repeats
       who + ": bot 1: " + noun + " 1" + walker_words);
  SAME(run(table(2, 3), {1, 0, 3}, 2, 3),   // and bot 0 before bot 2 leaves the records
       who + ": bot 0: " + noun + " 1" + walker_words);
  walker = -1;
  auto t = table(3, 2);
  t.front() = (T)kNaN;
  SAME(run(t, {0, 1}, 3, 3), who + ": row 0 holds a non-finite value");
  SAME(run(t, {0, 5}, 3, 3), who + ": bot 1: " + noun + " 5 is outside " + outside);   // two faults
  t.front() = (T)1, t.back() = (T)kInf;
  SAME(run(t, {0, 1}, 3, 3), who + ": row 2 holds a non-finite value");
  t[2 * L::kBotStride] = (T)kNaN;   // two faults: the first row in the table is named
  SAME(run(t, {0, 1}, 3, 3), who + ": row 1 holds a non-finite value");
}

// ---- dtdevbuf.h ------------------------------------------------------------
static const UploadCalls kCalls = {"alloc call", "sync call", "copy call"};

static bool holds(const DevBuf& b, const std::vector<int32_t>& v) {
  return b.ptr && memcmp(b.ptr, v.data(), v.size() * 4) == 0;
}

// dt_render_bots' sequence: the new table, then the drain and the column
// table in place, and only then the swap that frees the old table
static hipError_t replace(DevBuf& tab, DevBuf& col, const std::vector<int32_t>& t,
                          const std::vector<int32_t>& c, std::string& err) {
  DevBuf fresh;
  if (hipError_t e = upload_new(fresh, t.data(), t.size() * 4, "new alloc", "new copy", err)) return e;
  if (hipError_t e = upload_in_place(col, 64, c.data(), c.size() * 4, kCalls, err)) return e;
  tab = std::move(fresh);
  return hipSuccess;
}

static void buffer_cases() {
  std::string err;
  const std::vector<int32_t> small = {1, 2}, large = {3, 4, 5, 6, 7, 8, 9, 10}, other = {11, 12, 13};
  {
    // in place: one allocation of the capacity, the same pointer ever after
    DevBuf b;
    CHECK(upload_in_place(b, 32, nullptr, 0, kCalls, err) == hipSuccess);
    CHECK(!b.ptr && g_live == 0 && g_log == "s");   // nothing to copy: the drain alone
    CHECK(upload_in_place(b, 32, small.data(), 8, kCalls, err) == hipSuccess);
    void* const p = b.ptr;
    CHECK(p && b.bytes == 32 && g_live == 1 && g_log == "sms" && holds(b, small));
    CHECK(upload_in_place(b, 32, large.data(), 32, kCalls, err) == hipSuccess);
    CHECK(b.ptr == p && holds(b, large));
    CHECK(upload_in_place(b, 32, small.data(), 8, kCalls, err) == hipSuccess);
    CHECK(b.ptr == p && holds(b, small) && g_live == 1 && g_log == "smsss");
    // over the capacity: refused before any HIP call
    g_calls = 0;
    CHECK(upload_in_place(b, 32, large.data(), 36, kCalls, err) != hipSuccess);
    SAME(err, "copy call: injected");
    CHECK(g_calls == 0 && b.ptr == p && holds(b, small));
    // each HIP call failing in turn, on a buffer that holds a table
    const char* want[] = {"sync call: injected", "copy call: injected"};
    for (int k = 1; k <= 2; ++k) {
      g_calls = 0, g_fail_at = k;
      CHECK(upload_in_place(b, 32, other.data(), 12, kCalls, err) != hipSuccess);
      SAME(err, want[k - 1]);
      CHECK(b.ptr == p && holds(b, small) && g_live == 1);
    }
    // and on an empty one: a failed allocation leaves it empty
    DevBuf e;
    g_calls = 0, g_fail_at = 1;
    CHECK(upload_in_place(e, 32, other.data(), 12, kCalls, err) == hipErrorOutOfMemory);
    SAME(err, "alloc call: injected");
    CHECK(!e.ptr && e.bytes == 0 && g_live == 1);
    g_fail_at = 0;
  }
  CHECK(g_live == 0);
  {
    // replace: the new table is allocated before the old one is freed
    DevBuf tab, col;
    CHECK(replace(tab, col, small, other, err) == hipSuccess);
    CHECK(holds(tab, small) && holds(col, other) && g_live == 2);
    void* const old_tab = tab.ptr;
    void* const col_ptr = col.ptr;
    g_log.clear();
    CHECK(replace(tab, col, large, small, err) == hipSuccess);
    CHECK(g_log == "msf" && tab.ptr != old_tab && tab.bytes == 32 && holds(tab, large));
    CHECK(col.ptr == col_ptr && holds(col, small) && g_live == 2);
    // each HIP call failing in turn: the old table and the column table stay
    const char* want[] = {"new alloc: injected", "new copy: injected", "sync call: injected",
                          "copy call: injected"};
    void* const kept = tab.ptr;
    for (int k = 1; k <= 4; ++k) {
      g_calls = 0, g_fail_at = k;
      CHECK(replace(tab, col, other, other, err) != hipSuccess);
      SAME(err, want[k - 1]);
      CHECK(tab.ptr == kept && holds(tab, large) && col.ptr == col_ptr && holds(col, small));
      CHECK(g_live == 2);
    }
    // the column table's first allocation failing: it stays empty, the table unchanged
    DevBuf col2;
    g_calls = 0, g_fail_at = 3;
    CHECK(replace(tab, col2, other, other, err) == hipErrorOutOfMemory);
    SAME(err, "alloc call: injected");
    CHECK(tab.ptr == kept && holds(tab, large) && !col2.ptr && g_live == 2);
    g_fail_at = 0;
    // move-assignment frees what the target held; an empty source empties it
    g_log.clear();
    tab = DevBuf();
    CHECK(!tab.ptr && tab.bytes == 0 && g_live == 1 && g_log == "f");
    DevBuf moved(std::move(col));
    CHECK(moved.ptr == col_ptr && !col.ptr && g_live == 1);
    CHECK(moved.alloc(8) == hipErrorInvalidValue && moved.ptr == col_ptr);   // only of an empty buffer
  }
  CHECK(g_live == 0);
}

int main() {
  objects_cases();
  walker_cases<Step>("dt_set_walkers", "the handle's n_objects", " is a bot's row (dt_set_bots)");
  walker_cases<Frame>("dt_render_walkers", "the count dt_render_objects was given",
                          " is a render bot's record (dt_render_bots)");
  step_walker_cases();
  bot_cases<Step>("dt_set_bots", "n_objects", "object_row", "row", "n_objects",
                      " is a walker's row (dt_set_walkers)");
  bot_cases<Frame>("dt_render_bots", "the count dt_render_objects was given", "render_row",
                       "record", "dt_render_objects' count", " is a render walker's");
  buffer_cases();
  CHECK(g_live == 0);
  if (g_bad) fprintf(stderr, "%d check(s) failed\n", g_bad);
  return g_bad ? 1 : 0;
}
