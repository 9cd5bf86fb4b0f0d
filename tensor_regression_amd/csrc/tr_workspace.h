// tr_workspace.h — how a plan's workspace is declared (host only; no HIP here).
//
// One device allocation holds every buffer of a plan.  Its pieces are declared once, in order, each
// as the pointer that will address it plus a byte count; the same list gives the size to allocate
// (bytes()) and, once the allocation exists, the pointers into it (bind()).  Every piece starts
// 256 B aligned relative to the base.
#pragma once

#include <cstddef>
#include <cstring>
#include <vector>

namespace tr {

class Carver {
 public:
  // the next piece: *slot will address `bytes` bytes (rounded up to 256)
  template <class T>
  void add(T** slot, size_t bytes) {
    static_assert(sizeof(T*) == sizeof(void*), "object pointers only");
    pieces_.push_back({slot, total_, false});
    total_ += (bytes + 255) & ~(size_t)255;
  }
  // a piece some plans leave out: with bytes == 0 it takes no room and *slot binds to nullptr
  template <class T>
  void add_optional(T** slot, size_t bytes) {
    add(slot, bytes);
    pieces_.back().absent = bytes == 0;
  }
  size_t bytes() const { return total_; }
  // points every slot into the allocation at `base` (of at least bytes() bytes)
  void bind(void* base) const {
    for (const Piece& pc : pieces_) {
      void* at = pc.absent ? nullptr : static_cast<void*>(static_cast<char*>(base) + pc.offset);
      std::memcpy(pc.slot, &at, sizeof(at));  // (the slot is a T* of any object type T)
    }
  }

 private:
  struct Piece {
    void* slot;
    size_t offset;
    bool absent;
  };
  std::vector<Piece> pieces_;
  size_t total_ = 0;
};

}  // namespace tr
