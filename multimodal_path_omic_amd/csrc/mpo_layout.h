// Host-only: how the C-ABI entries cut a caller-owned buffer (`saved`, `workspace`) into tensors.
//
// A layout is written ONCE, as a function templated on the allocator that fills a struct of named pointers:
//     template <class A> FooWs foo_ws(A& a, geometry...) { return {a.floats(n0), a.floats(n1), ...}; }
// The size query runs it with Count, every entry that touches the buffer runs it with Carve, so a query and its entries
// cannot disagree.  Blocks are placed in the order of the braced list (its elements are evaluated left to right).
// The three placement rules below are the ones in use: offsets inside a buffer do not move.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

enum Placement {
    kWorkspace,   // every block starts at the next multiple of 256 bytes
    kPad64,       // every block is rounded up to 64 floats, so float4 accesses stay aligned (`saved` of the token tail)
    kPacked       // blocks follow one another (`saved` of the co-attention kernels)
};
constexpr size_t kWorkspaceSlack = 256;   // what a *_workspace_bytes() query adds to the end of its layout

// -> byte offset of a block of n floats placed after `end`, which moves behind the block
template <Placement P>
inline size_t place_block(size_t& end, size_t n) {
    const size_t o = P == kWorkspace ? (end + 255) / 256 * 256 : end;
    end = o + (P == kPad64 ? (n + 63) / 64 * 64 : n) * sizeof(float);
    return o;
}

// counts only
template <Placement P>
struct Count {
    using elem = float;
    size_t end = 0;
    float* floats(size_t n) { place_block<P>(end, n); return nullptr; }
    size_t n_floats() const { return end / sizeof(float); }
    size_t workspace_bytes() const { return end + kWorkspaceSlack; }
};

// hands out pointers into the caller's buffer; T = const float is a backward's view of `saved`.  A block that does not
// fit is nullptr and clears ok(): an entry checks ok() once, behind its layout function and before its first launch.
template <Placement P, typename T = float>
struct Carve {
    using elem = T;
    using Raw = typename std::conditional<std::is_const<T>::value, const void, void>::type;
    T* base;
    size_t size, end = 0;
    bool fits = true;
    explicit Carve(Raw* p, size_t bytes = SIZE_MAX) : base(static_cast<T*>(p)), size(bytes) {}   // (no length: `saved`)
    T* floats(size_t n) {
        size_t e = end;
        const size_t o = place_block<P>(e, n);
        if (e > size) { fits = false; return nullptr; }
        end = e;
        return base + o / sizeof(float);
    }
    bool ok() const { return fits; }
};

using WsCount = Count<kWorkspace>;
using WsCarve = Carve<kWorkspace>;
