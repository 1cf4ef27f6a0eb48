/* find_reject_count.c -- searches a Prio3Count helper measurement seed whose first candidate
 * element is rejected: the first 8 bytes of XOF(seed, dst(algorithm 0, usage 1), [agg_id 1]) --
 * TurboSHAKE128(0x08 || dst || seed || 0x01, D = 1) -- read little-endian are >= the Field64
 * modulus 2^64 - 2^32 + 1.  One seed in 2^32 does, so the search takes about 2^32 permutations.
 * It prints the seed (hex) that tests/golden/client_reject_count.json records as the first 16
 * bytes of the report's shard randomness.  Keccak-p[1600, 12] is the C restatement's.
 *
 *   make -C oracle
 *   gcc -O3 -march=x86-64-v3 -pthread -o /tmp/find_reject_count tools/find_reject_count.c \
 *       -Loracle/build -lprio3_oracle -Wl,-rpath,$PWD/oracle/build
 *   /tmp/find_reject_count [threads]
 *
 * Seed layout searched: bytes 0..7 a little-endian counter, byte 8 the thread, the rest zero
 * except the tag "reject" at bytes 10..15.  Which thread finds a seed first depends on timing;
 * any seed it prints is confirmed through the byte-level sponge before it is printed. */
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void orc_keccak_p1600(uint64_t st[25], int rounds);
void orc_turboshake128(const uint8_t* msg, size_t len, uint8_t domain, uint8_t* out, size_t out_len);

static const uint64_t P64 = 0xffffffff00000001ull;
static volatile int g_found = 0;
static uint8_t g_seed[16];
static pthread_mutex_t g_mu = PTHREAD_MUTEX_INITIALIZER;

static void make_msg(uint8_t msg[26], uint64_t ctr, uint8_t thread) {
  static const uint8_t head[9] = {8, /* dst: */ 8, 0, 0, 0, 0, 0, 0, 1};
  memcpy(msg, head, 9);
  memcpy(msg + 9, &ctr, 8); /* little-endian hosts only, like the restatement */
  msg[17] = thread;
  msg[18] = 0;
  memcpy(msg + 19, "reject", 6);
  msg[25] = 1; /* binder: agg_id */
}

static void* work(void* arg) {
  const uint8_t thread = (uint8_t)(uintptr_t)arg;
  uint8_t block[200];
  for (uint64_t ctr = 0; !g_found; ctr++) {
    uint64_t st[25];
    memset(block, 0, sizeof(block));
    make_msg(block, ctr, thread);
    block[26] = 0x01;   /* domain byte D = 1 */
    block[167] ^= 0x80; /* rate 168 */
    memcpy(st, block, 200);
    orc_keccak_p1600(st, 12);
    if (st[0] >= P64) {
      pthread_mutex_lock(&g_mu);
      if (!g_found) {
        memcpy(g_seed, block + 9, 16);
        g_found = 1;
      }
      pthread_mutex_unlock(&g_mu);
    }
  }
  return NULL;
}

int main(int argc, char** argv) {
  int nt = argc > 1 ? atoi(argv[1]) : 16;
  if (nt < 1 || nt > 255) nt = 16;
  pthread_t th[255];
  for (int i = 0; i < nt; i++) pthread_create(&th[i], NULL, work, (void*)(uintptr_t)i);
  for (int i = 0; i < nt; i++) pthread_join(th[i], NULL);
  /* confirm through the byte-level sponge */
  uint8_t msg[26], out[8];
  memcpy(msg, "\x08\x08\0\0\0\0\0\0\x01", 9);
  memcpy(msg + 9, g_seed, 16);
  msg[25] = 1;
  orc_turboshake128(msg, 26, 1, out, 8);
  uint64_t v;
  memcpy(&v, out, 8);
  if (v < P64) {
    fprintf(stderr, "internal error: candidate %016llx is below the modulus\n", (unsigned long long)v);
    return 1;
  }
  for (int i = 0; i < 16; i++) printf("%02x", g_seed[i]);
  printf(" first_candidate=%016llx\n", (unsigned long long)v);
  return 0;
}
