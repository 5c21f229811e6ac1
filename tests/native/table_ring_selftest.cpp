// Stand-alone check of ops/hip/table_ring.h, meant to be compiled with
// -fsanitize=address,undefined and run directly (see
// tests/test_table_ring.py). No HIP: completion is a callback, and this
// program plays the stream. Exit status 0 = every case passed.

#include <atomic>
#include <cstdio>
#include <stdexcept>
#include <thread>
#include <vector>

#include "table_ring.h"

using namespace tsamd;

namespace {

int g_failures = 0;

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failures;                                                      \
    }                                                                    \
  } while (0)

// What the callbacks saw, in order: +slot for an enqueue, -(slot + 1) for
// a wait.
struct Log {
  std::vector<int> calls;
  int waits = 0;
  int enqueues = 0;
};

bool launch(TableRing& ring, size_t bytes, Log& log) {
  return ring.launch(
      bytes,
      [&](int slot) {
        log.calls.push_back(-(slot + 1));
        ++log.waits;
      },
      [&](int slot) {
        log.calls.push_back(slot);
        ++log.enqueues;
      });
}

void fill_then_wrap() {
  TableRing ring(4, 1024);
  CHECK(ring.slots() == 4);
  CHECK(ring.slot_bytes() == 1024);
  Log log;
  // fill: every slot once, in order, no wait
  for (int i = 0; i < 4; ++i) CHECK(launch(ring, 100, log));
  CHECK(log.waits == 0);
  CHECK((log.calls == std::vector<int>{0, 1, 2, 3}));
  // wrap with the oldest slot still busy: wait on it, then reuse it
  CHECK(launch(ring, 1024, log));  // exactly a slot: fits
  CHECK(log.waits == 1);
  CHECK((log.calls == std::vector<int>{0, 1, 2, 3, -1, 0}));
  // and on round the ring: each reuse waits for its own slot first
  for (int i = 0; i < 7; ++i) CHECK(launch(ring, 8, log));
  CHECK(log.waits == 8 && log.enqueues == 12);
  const std::vector<int> tail(log.calls.end() - 4, log.calls.end());
  CHECK((tail == std::vector<int>{-3, 2, -4, 3}));
}

void oversized_takes_no_slot() {
  TableRing ring(2, 64);
  Log log;
  CHECK(launch(ring, 64, log));
  CHECK(!launch(ring, 65, log));  // fallback: nothing called
  CHECK(!launch(ring, (size_t)1 << 40, log));
  CHECK(log.enqueues == 1 && log.waits == 0);
  // the refusals did not advance the ring
  CHECK(launch(ring, 1, log));
  CHECK((log.calls == std::vector<int>{0, 1}));
}

void zero_length_is_a_table() {
  TableRing ring(2, 64);
  Log log;
  CHECK(launch(ring, 0, log));
  CHECK(launch(ring, 0, log));
  CHECK(launch(ring, 0, log));
  CHECK((log.calls == std::vector<int>{0, 1, -1, 0}));
  // a ring of zero-byte slots still carries zero-length tables
  TableRing none(1, 0);
  Log log2;
  CHECK(launch(none, 0, log2));
  CHECK(!launch(none, 1, log2));
  CHECK(log2.enqueues == 1);
}

void failed_launch_frees_the_slot() {
  TableRing ring(2, 64);
  Log log;
  bool threw = false;
  try {
    ring.launch(
        8, [&](int) { ++log.waits; },
        [&](int) { throw std::runtime_error("enqueue failed"); });
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw);
  // the same slot is handed out next, and without a wait
  CHECK(launch(ring, 8, log));
  CHECK((log.calls == std::vector<int>{0}) && log.waits == 0);
  // a failing wait leaves the slot busy: the next launch waits again
  CHECK(launch(ring, 8, log));  // slot 1
  threw = false;
  try {
    ring.launch(
        8, [&](int) { throw std::runtime_error("wait failed"); },
        [&](int) { ++log.enqueues; });
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw && log.enqueues == 2);
  CHECK(launch(ring, 8, log));
  CHECK((log.calls == std::vector<int>{0, 1, -1, 0}));
  bool no_slots = false;
  try {
    TableRing bad(0, 64);
  } catch (const std::invalid_argument&) {
    no_slots = true;
  }
  CHECK(no_slots);
}

// Eight launchers on one ring. The lock covers wait + enqueue, so the
// callbacks never overlap, slots go round in order, and a slot is never
// enqueued on twice without a wait in between.
void concurrent_launchers() {
  constexpr int kSlots = 4, kThreads = 8, kEach = 500;
  TableRing ring(kSlots, 64);
  std::atomic<int> inside{0};
  std::atomic<bool> overlapped{false};
  std::vector<int> in_flight(kSlots, 0);  // guarded by the ring's lock
  std::vector<int> order;
  bool reused_unwaited = false;
  std::vector<std::thread> threads;
  for (int t = 0; t < kThreads; ++t) {
    threads.emplace_back([&]() {
      for (int i = 0; i < kEach; ++i) {
        ring.launch(
            16,
            [&](int slot) {
              if (inside.fetch_add(1) != 0) overlapped = true;
              in_flight[slot] = 0;
              inside.fetch_sub(1);
            },
            [&](int slot) {
              if (inside.fetch_add(1) != 0) overlapped = true;
              if (in_flight[slot] != 0) reused_unwaited = true;
              in_flight[slot] = 1;
              order.push_back(slot);
              inside.fetch_sub(1);
            });
      }
    });
  }
  for (auto& th : threads) th.join();
  CHECK(!overlapped);
  CHECK(!reused_unwaited);
  CHECK(order.size() == (size_t)kThreads * kEach);
  bool round_robin = true;
  for (size_t i = 0; i < order.size(); ++i) {
    round_robin = round_robin && order[i] == (int)(i % kSlots);
  }
  CHECK(round_robin);
}

}  // namespace

int main() {
  fill_then_wrap();
  oversized_takes_no_slot();
  zero_length_is_a_table();
  failed_launch_frees_the_slot();
  concurrent_launchers();
  if (g_failures) {
    std::fprintf(stderr, "%d check(s) failed\n", g_failures);
    return 1;
  }
  std::printf("table_ring selftest OK\n");
  return 0;
}
