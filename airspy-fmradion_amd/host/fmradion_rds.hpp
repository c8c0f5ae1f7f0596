// fmradion_rds.hpp -- RDS block synchronisation, group assembly and a small parser (IEC 62106 / EN 50067 data link
// layer), header-only C++.  Input: the differentially decoded data bits of one RDS stream, in order, each with the
// absolute 384 kHz MPX sample index at which its symbol starts.  Output: groups of four 16-bit blocks with a status per
// block, in a bounded queue.
//
//   * 26-bit blocks: 16 information bits and a 10-bit checkword of g(x) = x^10 + x^8 + x^7 + x^5 + x^4 + x^3 + 1, to
//     which the offset word of the block's position is added (A 0x0FC, B 0x198, C 0x168, C' 0x350, D 0x1B4).
//   * Acquisition: two valid syndromes 26 bits apart whose offsets follow each other (A-B, B-C/C', C/C'-D, D-A); the
//     last valid syndrome is remembered per bit phase modulo 26, so a false one in between does not hide a true pair.
//   * Synchronised: every 26 bits one block of the expected position; a block whose syndrome is not that position's
//     offset is "bad".  kLoseSync bad blocks in a row drop the synchronisation, and acquisition starts again.
//   * Error detection only: no burst correction (the status value FMR_RDS_CORRECTED is never produced).
//   * A group is queued when its four positions have been received in synchronisation; a group whose acquisition
//     happened inside it after its block A is not queued (acquired on D-A, the A opens the next group).  A full queue drops its oldest group and counts it.
//
// The library runs one decoder per stream of a chain created with fmr_create_rds (include/fmradion_amd.h) on the bits its
// device stage hands over; it needs nothing but the C-ABI's record types, so a caller can also run it on bits of its own.
#pragma once
#include <cstddef>
#include <cstdint>
#include <deque>
#include <string>
#include <vector>

#include "../../include/fmradion_amd.h"

namespace fmr_rds {

constexpr uint16_t kOffsetA = 0x0FC, kOffsetB = 0x198, kOffsetC = 0x168, kOffsetCp = 0x350, kOffsetD = 0x1B4;
constexpr uint32_t kPoly = 0x5B9;           // g(x) = x^10 + x^8 + x^7 + x^5 + x^4 + x^3 + 1
constexpr int kLoseSync = 8;                // bad blocks in a row that drop the synchronisation (two groups)
constexpr size_t kQueueCap = 256;           // groups held per stream (~22 s of RDS)

// checkword of 16 information bits: m(x) x^10 mod g(x) (the offset word is added on top)
inline uint16_t checkword(uint16_t info) {
  uint32_t r = (uint32_t)info << 10;
  for (int b = 25; b >= 10; b--)
    if (r & (1u << b)) r ^= kPoly << (b - 10);
  return (uint16_t)(r & 0x3FF);
}

// syndrome of a received 26-bit block (bit 25 = the first bit on air) under the standard's parity-check matrix H: row i
// (for the i-th bit on air) is 1 << (9 - i) for the first ten bits, then the remainder of the following bits' columns,
// built by the feedback shift 0x2DC.  With it the offset words give the standard's syndromes (A 0x3D8, B 0x3D4, C 0x25C,
// C' 0x3CC, D 0x258); a codeword gives 0.
struct SyndromeTable {
  uint16_t t[4][256];
  SyndromeTable() {
    uint16_t row[26];
    row[0] = 0x200;
    for (int i = 1; i < 26; i++) row[i] = (uint16_t)((row[i - 1] >> 1) ^ ((row[i - 1] & 1) ? 0x2DC : 0));
    // byte j of the block (j = 0: bits 7..0, ... j = 3: bits 25..24)
    for (int j = 0; j < 4; j++)
      for (int v = 0; v < 256; v++) {
        uint16_t s = 0;
        for (int b = 0; b < 8; b++) {
          const int p = 8 * j + b;                 // bit position in the block
          if (p < 26 && (v >> b & 1)) s ^= row[25 - p];
        }
        t[j][v] = s;
      }
  }
};
inline uint16_t syndrome(uint32_t block26) {
  static const SyndromeTable tab;
  return (uint16_t)(tab.t[0][block26 & 0xFF] ^ tab.t[1][(block26 >> 8) & 0xFF] ^ tab.t[2][(block26 >> 16) & 0xFF] ^
                    tab.t[3][(block26 >> 24) & 0x03]);
}
inline uint16_t offset_syndrome(uint16_t offset) { return syndrome(offset); }

// position of a syndrome: 0 A, 1 B, 2 C, 3 C', 4 D; -1 none
inline int offset_of(uint16_t syn) {
  static const uint16_t s[5] = {offset_syndrome(kOffsetA), offset_syndrome(kOffsetB), offset_syndrome(kOffsetC),
                                offset_syndrome(kOffsetCp), offset_syndrome(kOffsetD)};
  for (int i = 0; i < 5; i++)
    if (syn == s[i]) return i;
  return -1;
}
inline int slot_of(int off) { return off <= 1 ? off : off == 4 ? 3 : 2; }   // group position 0..3 of an offset

class Decoder {
public:
  // one data bit (0 / 1) and the 384 kHz sample index of its symbol
  void push(int bit, uint64_t sample_index) {
    reg_ = ((reg_ << 1) | (uint32_t)(bit & 1)) & 0x3FFFFFFu;
    idx_[nbits_ % 32] = sample_index;
    nbits_++;
    if (nbits_ < 26) return;
    if (!synced_) { acquire(); return; }
    if (++in_block_ < 26) return;
    in_block_ = 0;
    const uint16_t info = (uint16_t)(reg_ >> 10);
    const int off = offset_of(syndrome(reg_));
    const int want = expect_;
    const bool ok = want == 2 ? (off == 2 || off == 3) : (off >= 0 && slot_of(off) == want);
    if (ok) {
      blocks_ok_++; bad_run_ = 0;
      store(want, info, off == 3 ? FMR_RDS_CPRIME : 0, first_index());
    } else {
      blocks_bad_++;
      store(want, info, FMR_RDS_BAD, first_index());
      if (++bad_run_ >= kLoseSync) { synced_ = false; have_ = 0; bad_run_ = 0; }
    }
    expect_ = (want + 1) & 3;
  }

  bool synced() const { return synced_; }
  uint64_t blocks_ok() const { return blocks_ok_; }
  uint64_t blocks_bad() const { return blocks_bad_; }
  uint64_t groups_dropped() const { return dropped_; }
  uint64_t groups_decoded() const { return decoded_; }
  size_t queued() const { return q_.size(); }
  // up to cap groups, oldest first, removed from the queue
  size_t pop(fmr_rds_group *out, size_t cap) {
    size_t n = 0;
    while (n < cap && !q_.empty()) { out[n++] = q_.front(); q_.pop_front(); }
    return n;
  }

private:
  uint64_t first_index() const { return idx_[(nbits_ - 26) % 32]; }
  // a valid syndrome is remembered per bit phase (mod 26): a false hit in between does not hide the true hit 26 bits back
  void acquire() {
    const int off = offset_of(syndrome(reg_));
    if (off < 0) return;
    const int slot = slot_of(off);
    Hit &h = hits_[nbits_ % 26];
    if (h.valid && nbits_ - h.at == 26 && ((h.slot + 1) & 3) == slot) {
      synced_ = true; in_block_ = 0; bad_run_ = 0; have_ = 0;
      blocks_ok_ += 2;
      if (h.slot == 0) store(0, h.info, 0, h.index);     // A-B: both blocks open the group
      if (h.slot == 0 || slot == 0) store(slot, (uint16_t)(reg_ >> 10), off == 3 ? FMR_RDS_CPRIME : 0, first_index());
      expect_ = (slot + 1) & 3;
      for (Hit &x : hits_) x.valid = false;
      return;
    }
    h = Hit{true, slot, (uint16_t)(reg_ >> 10), nbits_, first_index()};
  }
  void store(int slot, uint16_t info, uint8_t status, uint64_t index) {
    if (slot == 0) { have_ = 0; cur_ = fmr_rds_group{}; cur_.sample_index = index; }
    else if (!(have_ & (1u << (slot - 1)))) { have_ = 0; return; }   // the group did not start in synchronisation
    cur_.block[slot] = info;
    cur_.status[slot] = status;
    have_ |= 1u << slot;
    if (slot == 3 && have_ == 0xF) {
      if (q_.size() >= kQueueCap) { q_.pop_front(); dropped_++; }
      q_.push_back(cur_);
      decoded_++;
      have_ = 0;
    }
  }
  uint32_t reg_ = 0;
  uint64_t nbits_ = 0;
  uint64_t idx_[32] = {};
  bool synced_ = false;
  int in_block_ = 0, expect_ = 0, bad_run_ = 0;
  struct Hit { bool valid; int slot; uint16_t info; uint64_t at, index; };
  Hit hits_[26] = {};
  fmr_rds_group cur_{};
  unsigned have_ = 0;
  std::deque<fmr_rds_group> q_;
  uint64_t blocks_ok_ = 0, blocks_bad_ = 0, dropped_ = 0, decoded_ = 0;
};

// ---- parser: programme identification, programme type, programme service name (0A / 0B), RadioText (2A / 2B).  Only
// blocks whose status is FMR_RDS_OK (or corrected) are read.
inline bool block_ok(const fmr_rds_group &g, int i) { return (g.status[i] & FMR_RDS_BAD) == 0; }
inline int group_type(const fmr_rds_group &g) { return g.block[1] >> 12; }
inline int group_version_b(const fmr_rds_group &g) { return (g.block[1] >> 11) & 1; }

struct Station {
  int pi = -1;                       // -1: not yet seen
  int pty = -1;
  std::string ps = std::string(8, ' ');
  std::string rt = std::string(64, ' ');
  unsigned ps_seen = 0;              // bit per two-character segment of PS
  int rt_ab = -1;

  void add(const fmr_rds_group &g) {
    if (block_ok(g, 0)) pi = g.block[0];
    if (!block_ok(g, 1)) return;
    pty = (g.block[1] >> 5) & 0x1F;
    const int type = group_type(g), vb = group_version_b(g);
    if (type == 0 && block_ok(g, 3)) {
      const int seg = g.block[1] & 3;
      ps[2 * seg] = (char)(g.block[3] >> 8);
      ps[2 * seg + 1] = (char)(g.block[3] & 0xFF);
      ps_seen |= 1u << seg;
    } else if (type == 2) {
      const int ab = (g.block[1] >> 4) & 1;
      if (rt_ab >= 0 && ab != rt_ab) rt.assign(64, ' ');
      rt_ab = ab;
      const int seg = g.block[1] & 0xF;
      if (!vb && block_ok(g, 2) && block_ok(g, 3)) {
        rt[4 * seg] = (char)(g.block[2] >> 8); rt[4 * seg + 1] = (char)(g.block[2] & 0xFF);
        rt[4 * seg + 2] = (char)(g.block[3] >> 8); rt[4 * seg + 3] = (char)(g.block[3] & 0xFF);
      } else if (vb && block_ok(g, 3) && 2 * seg + 1 < 32) {
        rt[2 * seg] = (char)(g.block[3] >> 8); rt[2 * seg + 1] = (char)(g.block[3] & 0xFF);
      }
    }
  }
  bool ps_complete() const { return ps_seen == 0xF; }
};

}  // namespace fmr_rds
