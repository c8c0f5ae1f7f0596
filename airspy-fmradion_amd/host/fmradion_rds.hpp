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
//   * Error correction (set_correction; off by default), for synchronised blocks only -- acquisition always works on
//     uncorrected syndromes.  The error syndrome of a bad block is its syndrome xor the expected offset's syndrome.
//       burst  the error syndrome is looked up among all bursts of up to max_burst bits (1 .. 5, default 2; bursts of up
//              to five bits have distinct syndromes in this code, so a longer one is never taken for a shorter one).  A
//              wrong symbol gives two adjacent wrong bits after differential decoding: a burst of two.
//       soft   with a reliability |rho| per symbol (push with three arguments): of the 27 symbols the block's bits
//              depend on, the soft_symbols (1 .. 8, default 4) least reliable ones are tried in every non-empty
//              combination; flipping a symbol toggles its two bits (one, at either edge of the block).  The combination
//              that gives the expected syndrome at the smallest summed |rho| is taken if that sum is at most
//              soft_max_cost (default 1.0, one full symbol).  A block with a bit pushed without reliability is treated
//              in burst mode.
//     Position 3 takes C or C': the offset block B's version bit names if B is good or corrected, otherwise both, the
//     shorter burst / lower cost winning and a tie going to C.  A corrected block has status FMR_RDS_CORRECTED, counts in
//     blocks_corrected, and leaves the run of bad blocks as it is: it neither extends nor ends it, so miscorrected noise
//     cannot hold a false lock.
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
inline uint16_t syndrome_of_offset(int off) {
  static const uint16_t s[5] = {offset_syndrome(kOffsetA), offset_syndrome(kOffsetB), offset_syndrome(kOffsetC),
                                offset_syndrome(kOffsetCp), offset_syndrome(kOffsetD)};
  return s[off];
}

// every burst of up to kMaxBurst bits at every place of a 26-bit block, by its syndrome (all distinct): pattern and length
constexpr int kMaxBurst = 5, kMaxSoftSymbols = 8, kBlockSymbols = 27;
struct BurstTable {
  uint32_t pattern[1024];
  uint8_t length[1024];                     // 0: no burst of up to kMaxBurst bits has this syndrome
  bool distinct = true;
  BurstTable() {
    for (int i = 0; i < 1024; i++) { pattern[i] = 0; length[i] = 0; }
    for (int len = 1; len <= kMaxBurst; len++)
      for (uint32_t mid = 0; mid < (len > 2 ? 1u << (len - 2) : 1u); mid++) {
        const uint32_t shape = len == 1 ? 1u : (1u << (len - 1)) | (mid << 1) | 1u;
        for (int at = 0; at + len <= 26; at++) {
          const uint16_t syn = syndrome(shape << at);
          if (length[syn]) distinct = false;
          pattern[syn] = shape << at;
          length[syn] = (uint8_t)len;
        }
      }
  }
};
inline const BurstTable &burst_table() { static const BurstTable t; return t; }

struct Correction {                        // mode: FMR_RDS_FEC_*
  int mode = FMR_RDS_FEC_OFF, max_burst = 2, soft_symbols = 4;
  double soft_max_cost = 1.0;
};

class Decoder {
public:
  // one data bit (0 / 1) and the 384 kHz sample index of its symbol: no reliability
  void push(int bit, uint64_t sample_index) { push_bit(bit, sample_index, -1.f); }
  // ... with the symbol's reliability rho (its decision variable in units of the signal level; the sign is not read).
  // The bit also depends on the symbol before, whose reliability is that of the push before (or what carried() set).
  void push(int bit, uint64_t sample_index, float reliability) {
    const float a = reliability < 0.f ? -reliability : reliability;
    push_bit(bit, sample_index, a >= 0.f ? a : 0.f);                       // (NaN counts as unreliable)
  }
  // the reliability of the symbol before the next push, where the caller knows it better than the push before did
  void carried(float reliability) {
    const float a = reliability < 0.f ? -reliability : reliability;
    rel_[(nbits_ + 31) % 32] = a >= 0.f ? a : 0.f;
  }
  // error correction from the next block boundary on (while not synchronised: at once); false: out of range
  bool set_correction(const Correction &c) {
    if (c.mode != FMR_RDS_FEC_OFF && c.mode != FMR_RDS_FEC_BURST && c.mode != FMR_RDS_FEC_SOFT) return false;
    if (c.max_burst < 1 || c.max_burst > kMaxBurst || c.soft_symbols < 1 || c.soft_symbols > kMaxSoftSymbols) return false;
    if (!(c.soft_max_cost >= 0.0)) return false;
    next_ = c;
    if (!synced_ || in_block_ == 0) fec_ = next_;
    return true;
  }
  const Correction &correction() const { return next_; }

  bool synced() const { return synced_; }
  uint64_t blocks_ok() const { return blocks_ok_; }
  uint64_t blocks_bad() const { return blocks_bad_; }
  uint64_t blocks_corrected() const { return blocks_corrected_; }
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
  void push_bit(int bit, uint64_t sample_index, float rel) {
    reg_ = ((reg_ << 1) | (uint32_t)(bit & 1)) & 0x3FFFFFFu;
    idx_[nbits_ % 32] = sample_index;
    rel_[nbits_ % 32] = rel;
    nbits_++;
    if (nbits_ < 26) return;
    if (!synced_) { fec_ = next_; acquire(); return; }
    if (++in_block_ < 26) return;
    in_block_ = 0;
    const uint16_t info = (uint16_t)(reg_ >> 10);
    const int off = offset_of(syndrome(reg_));
    const int want = expect_;
    const bool ok = want == 2 ? (off == 2 || off == 3) : (off >= 0 && slot_of(off) == want);
    Fix fix;
    if (ok) {
      blocks_ok_++; bad_run_ = 0;
      store(want, info, off == 3 ? FMR_RDS_CPRIME : 0, first_index());
    } else if (fec_.mode != FMR_RDS_FEC_OFF && correct(want, fix)) {
      blocks_corrected_++;
      store(want, (uint16_t)((reg_ ^ fix.pattern) >> 10), FMR_RDS_CORRECTED | (fix.off == 3 ? FMR_RDS_CPRIME : 0), first_index());
    } else {
      blocks_bad_++;
      store(want, info, FMR_RDS_BAD, first_index());
      if (++bad_run_ >= kLoseSync) { synced_ = false; have_ = 0; bad_run_ = 0; }
    }
    expect_ = (want + 1) & 3;
    fec_ = next_;
  }

  struct Fix { uint32_t pattern = 0; int off = -1; double key = 0.0; };
  // the block in reg_ against offset `off`: the error pattern of the active mode and its key (burst length or cost)
  bool fix_for(int off, bool soft, Fix &f) const {
    const uint16_t es = (uint16_t)(syndrome(reg_) ^ syndrome_of_offset(off));
    f.off = off;
    if (!soft) {
      const BurstTable &t = burst_table();
      if (t.length[es] == 0 || t.length[es] > fec_.max_burst) return false;
      f.pattern = t.pattern[es]; f.key = t.length[es];
      return true;
    }
    // symbol j = 0 .. 26 of the block: the one before its first bit, then the symbols of its 26 bits; its reliability
    // is that of push nbits_ - 27 + j, and flipping it toggles the bits on air j - 1 and j (bit on air i = bit 25 - i)
    int pick[kMaxSoftSymbols];
    const int m = fec_.soft_symbols;
    bool used[kBlockSymbols] = {};
    for (int q = 0; q < m; q++) {                       // the m least reliable, the earlier symbol first among equals
      int best = -1;
      for (int j = 0; j < kBlockSymbols; j++)
        if (!used[j] && (best < 0 || rel_at(j) < rel_at(best))) best = j;
      used[best] = true; pick[q] = best;
    }
    uint32_t pat[kMaxSoftSymbols]; uint16_t syn[kMaxSoftSymbols];
    for (int q = 0; q < m; q++) {
      const int j = pick[q];
      pat[q] = (j >= 1 ? 1u << (26 - j) : 0u) | (j <= 25 ? 1u << (25 - j) : 0u);
      syn[q] = syndrome(pat[q]);
    }
    bool found = false;
    for (unsigned mask = 1; mask < (1u << m); mask++) {
      uint16_t sy = 0; uint32_t p = 0; double cost = 0.0;
      for (int q = 0; q < m; q++)
        if (mask >> q & 1) { sy ^= syn[q]; p ^= pat[q]; cost += (double)rel_at(pick[q]); }
      if (sy != es || (found && !(cost < f.key))) continue;
      found = true; f.pattern = p; f.key = cost;
    }
    return found && f.key <= fec_.soft_max_cost;
  }
  float rel_at(int j) const { return rel_[(nbits_ - 27 + j) % 32]; }
  bool correct(int want, Fix &best) const {
    bool soft = fec_.mode == FMR_RDS_FEC_SOFT;
    if (soft) {
      if (nbits_ < 27) soft = false;
      for (int j = 0; soft && j < kBlockSymbols; j++)
        if (rel_at(j) < 0.f) soft = false;               // a bit without reliability: burst mode for this block
    }
    if (want != 2) return fix_for(want == 3 ? 4 : want, soft, best);
    // C or C': what a good (or corrected) block B says, otherwise both; the smaller key wins, a tie goes to C
    const bool b_known = (have_ & 2u) && !(cur_.status[1] & FMR_RDS_BAD);
    const bool ver_b = b_known && ((cur_.block[1] >> 11) & 1);
    Fix c, cp;
    const bool hc = (!b_known || !ver_b) && fix_for(2, soft, c);
    const bool hp = (!b_known || ver_b) && fix_for(3, soft, cp);
    if (!hc && !hp) return false;
    best = hc && (!hp || c.key <= cp.key) ? c : cp;
    return true;
  }
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
  float rel_[32] = {};                       // |rho| of the symbol of each bit; < 0: pushed without reliability
  Correction fec_, next_;                    // in force for the block being received; from the next block boundary
  bool synced_ = false;
  int in_block_ = 0, expect_ = 0, bad_run_ = 0;
  struct Hit { bool valid; int slot; uint16_t info; uint64_t at, index; };
  Hit hits_[26] = {};
  fmr_rds_group cur_{};
  unsigned have_ = 0;
  std::deque<fmr_rds_group> q_;
  uint64_t blocks_ok_ = 0, blocks_bad_ = 0, blocks_corrected_ = 0, dropped_ = 0, decoded_ = 0;
};

// ---- parser: programme identification, programme type, programme service name (0A / 0B), RadioText (2A / 2B).  Only
// blocks whose status is FMR_RDS_OK or FMR_RDS_CORRECTED are read.
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
