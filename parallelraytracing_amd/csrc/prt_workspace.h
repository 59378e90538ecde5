// prt_workspace.h — where a call's arrays lie in one device buffer.  HIP-free; included by the .cpp units only.
//
// A caller declares its arrays in order (add: a typed pointer and an element count), asks for bytes() to size the buffer,
// and binds the layout to (base, capacity), which fills in the declared pointers.  The total and the pointers come from
// the same declarations, so an array added later cannot be left out of the size.  Every array starts on a multiple of
// 16 bytes from the base; base itself may be any 16-byte aligned address inside a larger allocation.
#pragma once

#include <cstddef>
#include <cstring>

struct PrtWorkspace {
    static constexpr int kMaxRegions = 48;  // (the lit bake with textures and the texel's light sample declares 33)

    // Declares `count` elements of T behind *p, after everything declared before.  *p is null until bind succeeds.
    template <class T>
    PrtWorkspace& add(T** p, size_t count) {
        *p = nullptr;
        if (n_ == kMaxRegions) {
            overflow_ = true;
            return *this;
        }
        slot_[n_] = p;
        off_[n_] = total_;
        ++n_;
        total_ = (total_ + count * sizeof(T) + 15) & ~(size_t)15;
        return *this;
    }

    // Bytes a buffer needs to hold every declared array: the end of the last one, rounded up to 16.
    size_t bytes() const { return total_; }
    int regions() const { return n_; }
    size_t offset(int i) const { return off_[i]; }

    // Fills in the declared pointers from base.  False, with every pointer null, if the layout does not fit in `capacity`
    // bytes, has no buffer to lie in, or declared more arrays than kMaxRegions.
    bool bind(void* base, size_t capacity) const {
        const bool ok = !overflow_ && total_ <= capacity && (base || !total_);
        for (int i = 0; i < n_; ++i) {
            char* p = ok ? (char*)base + off_[i] : nullptr;
            memcpy(slot_[i], &p, sizeof(p));  // (slot_[i] is a T**: every object pointer has void*'s representation here)
        }
        return ok;
    }

private:
    void* slot_[kMaxRegions] = {};
    size_t off_[kMaxRegions] = {};
    size_t total_ = 0;
    int n_ = 0;
    bool overflow_ = false;
};
