// Slot policy of the launch-table ring.
//
// Every gather / scatter launch uploads one small table (descriptors and
// prefix sums, LaunchTables in desc_check.h) that its kernel reads. The
// table travels through a ring of fixed slots, one ring per device and per
// side stream: a slot is a pinned host buffer, a device buffer of the same
// size and an event recorded behind the kernel that reads the device half.
// The upload is then a copy out of pinned memory, which the runtime really
// does enqueue and return from; out of pageable memory it waits for
// everything queued on the stream before it.
//
// This header is the policy alone: which slot a launch takes, when it has
// to wait for that slot's previous user, and when a table does not go
// through the ring at all. Plain C++17: no HIP, no pybind, so it builds
// stand-alone (tests/native/table_ring_selftest.cpp runs it under the host
// sanitizers). Completion is a callback; staging.hip supplies the HIP
// calls.
//
// Rules:
//   - slots are handed out round-robin. All launches of a ring go to one
//     stream, so the oldest slot is also the first to complete
//   - a slot is taken again only after wait_slot(slot) has returned for its
//     previous use. A slot that was never used, or whose launch failed, is
//     taken without waiting
//   - a table larger than a slot takes no slot: launch() returns false and
//     touches nothing, and the caller uploads it some other way
//   - a table of zero bytes is a table like any other: it takes a slot
//   - the ring's lock is held from the choice of the slot until enqueue()
//     returns, so concurrent launchers cannot interleave their "copy, then
//     kernel, then event", and a slot's event is recorded before anyone
//     can come round to wait on it

#pragma once

#include <cstddef>
#include <mutex>
#include <stdexcept>
#include <vector>

namespace tsamd {

constexpr int kTableRingSlots = 16;
// 64 KiB holds the tables of about 540 descriptors; the flagship's slabs
// have about ten
constexpr size_t kTableRingSlotBytes = 64 * 1024;

class TableRing {
 public:
  TableRing(int slots, size_t slot_bytes)
      : slot_bytes_(slot_bytes), busy_(slots > 0 ? slots : 0, false) {
    if (slots <= 0) throw std::invalid_argument("TableRing: no slots");
  }

  int slots() const { return (int)busy_.size(); }
  size_t slot_bytes() const { return slot_bytes_; }

  // One launch whose table has `table_bytes` bytes. Returns false when the
  // table does not fit a slot (nothing was called, nothing changed).
  // Otherwise calls wait_slot(slot) if the slot's previous launch may still
  // be running, then enqueue(slot), and returns true.
  //
  // enqueue(slot) fills the slot's host half, enqueues copy, kernel and the
  // slot's event record. If it throws, it must leave nothing of its own in
  // flight on the slot; the slot then stays free and is the next one handed
  // out. If wait_slot throws, the slot stays busy.
  template <typename WaitSlot, typename Enqueue>
  bool launch(size_t table_bytes, WaitSlot&& wait_slot, Enqueue&& enqueue) {
    if (table_bytes > slot_bytes_) return false;
    std::lock_guard<std::mutex> lk(mu_);
    const int slot = next_;
    if (busy_[slot]) {
      wait_slot(slot);
      busy_[slot] = false;
    }
    enqueue(slot);
    busy_[slot] = true;
    next_ = (slot + 1) % (int)busy_.size();
    return true;
  }

 private:
  const size_t slot_bytes_;
  std::mutex mu_;
  std::vector<bool> busy_;  // an event record is outstanding on the slot
  int next_ = 0;
};

}  // namespace tsamd
