// pcp_tables.h — the model tables as the kernels read them: formats and limits only, no HIP header.  Shared between the host-side
// lowering (pcp_lower.hip), the C-ABI host code (pcp_api.hip) and, through pcp_internal.h, the gfx950 kernels.
#pragma once
#include <stdint.h>

namespace pcp {

// One elementary filter as the kernels see it: 16 bytes, one dwordx4 load per lane.
//   xk : operand-x slot | kind << 28          (slot = index into the node's extended domain array)
//   y,z: operand slots (z unused for binary kinds)
//   d  : the single folded offset.  Binary kinds relate  X = dom[x]  and  Y = dom[y] + d.
//        Ternary kinds relate  x  and  y + z + d.   (EQ3: geq uses d-1, leq uses d+1.)
// Constants are interned as pseudo-variables in slots [n_vars, n_slots): their domain is the singleton
// {c}; narrowing it empties it, which is exactly Constant::update returning false (term/constant.rs:49-52).
struct __attribute__((aligned(16))) Rec {
  uint32_t xk;
  uint32_t y;
  uint32_t z;
  int32_t d;
};
static_assert(sizeof(Rec) == 16, "Rec must be 16 bytes");

constexpr uint32_t kSlotMask = 0x0FFFFFFFu;
constexpr uint32_t kMaxSlots = 1u << 26;  // (node, slot) pairs are packed into 32 bits in the kernels

// Compact 8-byte form of a binary record, used for the sweep's stream when every record of the model is binary and
// every slot index fits 15 bits (always true when the domains are LDS-resident with B > 1): the stream, which every
// workgroup reads in full, is half as long.   x = slot_x | slot_y << 15 | kind << 30,   y = d.
struct __attribute__((aligned(8))) Rec8 {
  uint32_t xyk;
  int32_t d;
};
static_assert(sizeof(Rec8) == 8, "Rec8 must be 8 bytes");
constexpr uint32_t kCompactSlots = 1u << 15;

// Word descriptor for the sweep's level -1 test (packed tiles): what the 64 records of one live-mask word have in
// common.  cls = 1 (all XNeqY) or 2 (all XLessY) when the operand slots of the word span at most kRangeMax consecutive
// slots each and every offset fits 16 bits, else 0 (the word always goes to the record-level tests).  A slot range
// [lo, hi] is queried in the tile's range-minimum tables as min(T[k][lo], T[k][second]) with 2^k <= hi-lo+1 < 2^(k+1).
struct __attribute__((aligned(16))) WordPart {
  uint32_t x;  // xlo | second_x << 16
  uint32_t y;  // ylo | second_y << 16
  uint32_t k;  // kx | ky << 4 | cls << 8 | (part b present) << 12
  uint32_t d;  // (dmin & 0xffff) | dmax << 16     (int16 each)
};
// A word that straddles two x-blocks of a table sorted by x (its y operands jump back) is described as two parts, the
// records before and after the first change of x; the word passes level -1 when both parts do.
struct __attribute__((aligned(16))) WordDesc {
  WordPart a, b;
};
static_assert(sizeof(WordDesc) == 32, "WordDesc must be 32 bytes");
// Group descriptor (implicit nodes): what the 64 words = 4096 records of one GROUP have in common, for a test one level above the
// word test: x slots within a short range (as in WordPart), y slots somewhere in [ylo, n_slots) — queried as a SUFFIX minimum —
// and offsets in [dmin, dmax].  cls as in WordPart (0 = no group test).
struct __attribute__((aligned(16))) GroupDesc {
  uint32_t x;    // xlo | second_x << 16
  uint32_t k;    // kx | cls << 8
  uint32_t ylo;  // smallest y slot of the group
  uint32_t d;    // (dmin & 0xffff) | dmax << 16
};
static_assert(sizeof(GroupDesc) == 16, "GroupDesc must be 16 bytes");
constexpr uint32_t kRangeMax = 64;    // longest slot range a descriptor may cover
constexpr uint32_t kRangeLevels = 7;  // table levels 2^0 .. 2^6

// Both record tables are padded with copies of their last record up to a multiple of 256 records plus kStreamPadRecs, so
// that the sweep's unconditional prefetch (up to two rounds of 16 wavefronts x 4 words ahead) needs no index clamping.
constexpr uint32_t kStreamPadRecs = 2 * 16 * 4 * 64;

constexpr int32_t kPackedMax = 16383;   // |bound| limit of the packed tiles: sums of two bounds fit int16
constexpr int kBoundMax = (1 << 29) - 1;  // the engine's arithmetic (sums of two bounds and an offset) is exact for |bound| <= kBoundMax

// The 8-byte payload tables (ModelDev::adjp; BigRec / BigAdj, pcp_neq.h) are uint2 on the device; the host side builds them as this.
struct __attribute__((aligned(8))) U32x2 {
  uint32_t x, y;
};
static_assert(sizeof(U32x2) == 8 && alignof(U32x2) == 8, "U32x2 must match the device's uint2");

}  // namespace pcp
