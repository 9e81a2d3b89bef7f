/* rds_check.c - drives csrc/fmd_rds.c alone (no GPU header, no library: the unit is device-free), built by tests/test_rds_cpu.py with
 * AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program.  Every check prints one line; the exit status is the number of failed
 * checks.  What it walks: the range check and geometry over every rate the range admits at five block lengths (the edges included), the tap
 * design and timing table at their largest sizes, the decoder over a synthesised bit stream in every split (whole, bit by bit, random pieces, a full output array), garbage, flipped bits, a
 * dropped bit (sync loss and re-acquisition) and the PS collector. */
#define _GNU_SOURCE
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fmd_internal.h"

int fmd_fail(int code, const char *fmt, ...) { (void)fmt; return code; }

static int failed;
#define CHECK(cond, ...) do { const int ok_ = (cond); printf("%s: ", ok_ ? "ok  " : "FAIL"); printf(__VA_ARGS__); printf("\n"); failed += !ok_; } while (0)

static uint32_t lcg_state = 12345;
static uint32_t lcg(void) { lcg_state = 1664525u * lcg_state + 1013904223u; return lcg_state >> 8; }

static const uint16_t offs[5] = {0x0FC, 0x198, 0x168, 0x1B4, 0x350};
static uint32_t rem26(uint32_t w) {
  for (int i = 25; i >= 10; i--)
    if (w & (1u << i)) w ^= 0x5B9u << (i - 10);
  return w & 0x3FFu;
}

/* 104 soft bits of a group (-1 for a 1), first transmitted first */
static void group_soft(const uint16_t blk[4], int version_b, float *out) {
  for (int p = 0; p < 4; p++) {
    const uint32_t info = (uint32_t)blk[p] << 10;
    const uint32_t w = info | (rem26(info) ^ offs[p == 2 && version_b ? 4 : p]);
    for (int i = 0; i < 26; i++) out[26 * p + i] = ((w >> (25 - i)) & 1u) ? -1.0f : 1.0f;
  }
}

#define NG 40
static uint16_t sent[NG][4];
static float stream[NG * 104];

static void make_stream(void) {
  const char *ps = "RDS TEST";
  for (int g = 0; g < NG; g++) {
    const int seg = g & 3, vb = (g % 5) == 4;
    sent[g][0] = 0xD3A5;
    sent[g][1] = (uint16_t)((vb << 11) | (9 << 5) | seg);
    sent[g][2] = vb ? 0xD3A5 : (uint16_t)(0xE000 + g);
    sent[g][3] = (uint16_t)(((uint8_t)ps[2 * seg] << 8) | (uint8_t)ps[2 * seg + 1]);
    group_soft(sent[g], vb, stream + 104 * g);
  }
}

/* push `n` soft bits in pieces (piece(i) gives the next length), collecting into out; returns the number of groups */
static int push_split(fmd_rds_decoder *d, const float *soft, int n, int mode, fmd_rds_group *out, int cap) {
  int got = 0, at = 0;
  while (at < n) {
    int len = mode == 0 ? n : mode == 1 ? 1 : 1 + (int)(lcg() % 61);
    if (len > n - at) len = n - at;
    const int room = mode == 3 ? 1 : cap - got;              /* mode 3: an output array of one group, so the call stops early */
    const int k = fmd_rds_decoder_push(d, soft + at, len, out + got, room);
    if (k < 0 || k > room) return -1;
    got += k;
    at += d->consumed;
    if (d->consumed == 0 && k == 0 && room > 0) return -2;  /* no progress */
  }
  return got;
}

static int same_groups(const fmd_rds_group *a, const fmd_rds_group *b, int n) {
  for (int i = 0; i < n; i++)
    if (memcmp(a[i].blk, b[i].blk, sizeof(a[i].blk)) || a[i].ok_mask != b[i].ok_mask || a[i].version != b[i].version) return 0;
  return 1;
}

int main(void) {
  /* 1. range, geometry, taps, table */
  int n_ok = 0, most_pw = 0, most_hy = 0, full_slots = 0;
  /* block lengths: the middle of the range, then the edges the GPU edge tests run at - the shortest block the longest lookback admits, a block of
   * 4 bits at S = 32, the first block of more than 256 bits at S = 10, and the longest */
  static const int block_zs[] = {4096, 68, 128, 2816, FMDK_RDS_MAX_BLOCK};
  for (size_t bi = 0; bi < sizeof(block_zs) / sizeof(block_zs[0]); bi++)
  for (int rz = 125; rz <= 40000; rz += 125) {
    fmd_rds_config c = {rz, block_zs[bi], 64, 8, 4};
    if (fmdk_rds_check(&c) != FMD_OK) continue;
    n_ok += bi == 0;
    fmdk_rds_geom g;
    fmdk_rds_geometry(rz, c.block_z, &g);
    float taps[FMD_RDS_MAX_TAPS], tab[2 * FMD_RDS_MAX_PERIOD];
    if (fmd_rds_design(&c, taps) != FMD_OK) failed++;
    fmdk_rds_table(&c, tab);
    if (g.pw > FMD_RDS_MAX_PERIOD || g.pw > 640 || g.hy > FMD_RDS_MAX_YHIST || g.hy > 68 || g.hy > c.block_z || 2375 * g.lb >= g.two_rz ||
        g.slot * (long long)g.two_rz < 2375LL * c.block_z)
      failed++;
    if (g.pw > most_pw) most_pw = g.pw;
    if (g.hy > most_hy) most_hy = g.hy;
    /* ownership: counts over many blocks add up to the nominal count, every count fits the slot */
    long long e = 2375LL * g.lb, bits = 0, most = 0;
    const int nb = 1000;
    for (int b = 0; b < nb; b++) {
      const long long lim = 2375LL * c.block_z, cnt = e < lim ? (lim - e + g.two_rz - 1) / g.two_rz : 0;
      if (cnt > g.slot || e < 0 || e >= g.two_rz) failed++;
      if (cnt > most) most = cnt;
      bits += cnt;
      e += cnt * g.two_rz - lim;
    }
    /* nominal: the bits k >= 0 with k S < nb Bz - L */
    const long long span = 2375LL * ((long long)nb * c.block_z - g.lb), nominal = (span + g.two_rz - 1) / g.two_rz;
    if (bits != nominal) failed++;
    full_slots += most == g.slot;
    /* the largest values the slicer forms in 32-bit integers: E = e0 + (j - m) 2 rate_z with e0 < 2375 (Bz + Hb) + 2 rate_z, j < slot */
    if (2375LL * (c.block_z + g.hb) + (long long)(g.slot + 1) * g.two_rz > 0x7fffffffLL) failed++;
  }
  CHECK(n_ok == (38000 - 11875) / 125 + 1 && !failed, "range: %d rates admitted, geometry, taps and table made for each at %d block lengths", n_ok,
        (int)(sizeof(block_zs) / sizeof(block_zs[0])));
  CHECK(most_pw == 606 && most_hy == 66 && full_slots > 0, "range: the longest timing period %d of %d, the longest lookback %d of %d, %d geometries whose slot fills",
        most_pw, FMD_RDS_MAX_PERIOD, most_hy, FMD_RDS_MAX_YHIST, full_slots);
  {
    fmd_rds_config bad[] = {{18750, 62, 64, 8, 4}, {18750, 64, 68, 8, 4}, {18751, 64, 64, 8, 4}, {9000, 64, 16, 8, 4}, {40000, 256, 64, 8, 4},
                            {18750, 32, 16, 8, 4}, {18750, 64, 64, 0, 4}, {18750, 64, 64, 8, 0}, {18750, 64, 12, 8, 4}};
    int refused = 0;
    for (size_t i = 0; i < sizeof(bad) / sizeof(bad[0]); i++) refused += fmdk_rds_check(&bad[i]) == FMD_E_UNSUPPORTED;
    CHECK(refused == 9 && fmdk_rds_check(NULL) == FMD_E_ARG, "range: %d of 9 bad configurations refused", refused);
  }

  /* 2. the decoder: every split gives the same groups */
  make_stream();
  static fmd_rds_group ref[NG + 2], got[NG + 2];
  fmd_rds_decoder d;
  fmd_rds_decoder_init(&d);
  const int n_ref = push_split(&d, stream, NG * 104, 0, ref, NG + 2);
  int all_full = n_ref == NG;
  for (int g = 0; g < n_ref && g < NG; g++)
    all_full &= ref[g].ok_mask == 15 && !memcmp(ref[g].blk, sent[g], 8) && ref[g].version == (g % 5 == 4);      /* (block A of the first: taken when B confirms it) */
  CHECK(all_full && d.synced && d.n_sync == 1 && d.n_loss == 0, "whole stream: %d groups of %d, all blocks ok", n_ref, NG);
  for (int mode = 1; mode <= 3; mode++)
    for (int rep = 0; rep < (mode == 2 ? 20 : 1); rep++) {
      fmd_rds_decoder_init(&d);
      const int n = push_split(&d, stream, NG * 104, mode, got, NG + 2);
      if (n != n_ref || !same_groups(ref, got, n_ref)) { CHECK(0, "split mode %d rep %d: %d groups", mode, rep, n); }
    }
  CHECK(1, "splits: bit by bit, 20 random splits, one-group output arrays");

  /* 3. garbage: whatever it does, it stays in bounds; the counters are consistent */
  {
    static float junk[100000];
    for (int i = 0; i < 100000; i++) junk[i] = (lcg() & 1) ? -0.5f : 0.5f;
    fmd_rds_decoder_init(&d);
    static fmd_rds_group many[1000];
    const int n = push_split(&d, junk, 100000, 2, many, 1000);
    CHECK(n >= 0 && d.bits == 100000 && d.n_loss <= d.n_sync, "garbage: 100000 random bits, %d groups, %u acquisitions", n, d.n_sync);
  }

  /* 4. one flipped bit per group, in turn in each block: that block alone is bad, nothing wrong comes out */
  {
    static float s2[NG * 104];
    memcpy(s2, stream, sizeof(s2));
    for (int g = 2; g < NG; g++) s2[104 * g + 26 * (g & 3) + (int)(lcg() % 26)] *= -1.0f;
    fmd_rds_decoder_init(&d);
    const int n = push_split(&d, s2, NG * 104, 2, got, NG + 2);
    int good = n == NG;
    for (int g = 2; g < n && g < NG; g++) {
      good &= got[g].ok_mask == (15 & ~(1 << (g & 3)));
      for (int p = 0; p < 4; p++)
        if (got[g].ok_mask & (1 << p)) good &= got[g].blk[p] == sent[g][p];
    }
    CHECK(good && d.n_loss == 0, "flipped bits: each marked its block bad, %d groups, no wrong block", n);
  }

  /* 5. a dropped bit: FMD_RDS_SYNC_LOSS bad blocks, sync lost, acquired again; every group that comes out whole is one that was sent */
  {
    static float s3[NG * 104];
    const int cut = 104 * 10 + 37;
    memcpy(s3, stream, sizeof(float) * (size_t)cut);
    memcpy(s3 + cut, stream + cut + 1, sizeof(float) * (size_t)(NG * 104 - cut - 1));
    fmd_rds_decoder_init(&d);
    const int n = push_split(&d, s3, NG * 104 - 1, 2, got, NG + 2);
    int whole = 0, wrong = 0, next = 0;
    for (int i = 0; i < n; i++) {
      if (got[i].ok_mask != 15) continue;
      int at = -1;
      for (int g = next; g < NG; g++)
        if (!memcmp(got[i].blk, sent[g], 8)) { at = g; break; }
      if (at < 0) wrong++; else { whole++; next = at + 1; }
    }
    CHECK(d.n_sync == 2 && d.n_loss == 1 && d.synced && !wrong && whole >= NG - 5, "dropped bit: lost and re-acquired, %d of %d groups whole, %d wrong", whole, NG, wrong);
  }

  /* 6. PI, PTY, PS */
  {
    fmd_rds_info info;
    fmd_rds_info_init(&info);
    fmd_rds_group bad = ref[1];
    bad.ok_mask = 7;                                          /* block D not ok: its characters must not be taken */
    bad.blk[3] = 0x5858;
    fmd_rds_info_update(&info, &bad);
    const int none = info.ps_mask == 0 && info.have_pi && info.pi == 0xD3A5 && info.pty == 9;
    for (int g = 0; g < n_ref; g++) fmd_rds_info_update(&info, &ref[g]);
    CHECK(none && info.ps_mask == 15 && !strcmp(info.ps, "RDS TEST"), "info: PI %04X PTY %d PS \"%s\"", info.pi, info.pty, info.ps);
    /* no room for a group: out of sync no bit is taken (any bit could acquire at position D and emit), in sync all but a group's last bit */
    fmd_rds_decoder_init(&d);
    const int k0 = fmd_rds_decoder_push(&d, stream, 104, NULL, 0), c0 = d.consumed;
    fmd_rds_group one[1];
    const int k1 = fmd_rds_decoder_push(&d, stream, 104, one, 1), c1 = d.consumed, synced = d.synced;
    const int k2 = fmd_rds_decoder_push(&d, stream + 104, 208, NULL, 0), c2 = d.consumed;
    CHECK(k0 == 0 && c0 == 0 && k1 == 1 && c1 == 104 && synced && k2 == 0 && c2 == 103 && d.bits == 207, "no room: %d bits taken out of sync, %d in sync", c0, c2);
    CHECK(fmd_rds_info_update(NULL, &bad) == 0 && fmd_rds_decoder_push(NULL, NULL, 0, NULL, 0) == FMD_E_ARG, "NULL arguments refused");
  }
  printf("%d checks failed\n", failed);
  return failed;
}
