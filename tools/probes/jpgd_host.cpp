// Stand-alone run of the JPEG decoder's rule on the host (csrc/jpgd_rule.hpp through csrc/jpgd_plan.hpp's host path), for a
// sanitizer build: no HIP, no Python.
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/probes/jpgd_host.cpp -o jpgd_host
//   jpgd_host [--selftest] [--mangle] [--sync S | --split S] file.jpg ...
// Every file is planned and decoded as given; FILE.rgb beside it, when present, must hold the decoded bytes (host_models.
// jpeg_decode_rgb8's).  --mangle: also every file cut at 64 places and with a bit flipped at 256 places, header and scan alike:
// a refusal by the plan or a decode with a status word, never an access outside the file's bytes.  Each mangled copy lives in a
// heap block of exactly its size, so that the sanitizer sees one byte too far.  --sync S (before the files): every decode runs a
// second time with the sync entropy route and subsequences of S bytes, and must give the interval route's bytes and status word;
// --split S: the same with the split route, which also takes files with restart markers.
#include <stdlib.h>

#include <string>

#include "../../comfyui-float_optimized_amd/csrc/jpgd_plan.hpp"

static std::vector<uint8_t> slurp(const std::string& path) {
  std::vector<uint8_t> v;
  if (FILE* f = fopen(path.c_str(), "rb")) {
    uint8_t buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) v.insert(v.end(), buf, buf + n);
    fclose(f);
  }
  return v;
}

static int g_sync = 0, g_sync_differs = 0, g_entropy = 1;

// 0 decoded, 1 refused; rgb and status filled when decoded
static int decode(const uint8_t* bytes, size_t n, std::vector<uint8_t>* rgb, int32_t* status, std::string* why) {
  uint8_t* exact = (uint8_t*)malloc(n ? n : 1);  // no slack behind the file
  memcpy(exact, bytes, n);
  const int64_t offsets[2] = {0, (int64_t)n};
  std::vector<int32_t> plan(jpgd_plan_ints(1));
  char err[400] = "";
  const int rc = jpgd_build_plan(exact, offsets, 1, plan.data(), plan.size(), err, sizeof(err));
  if (rc == 0) {
    rgb->assign((size_t)plan[JPGD_P_H] * plan[JPGD_P_W] * 3, 0);
    jpgd_host_frame(exact, offsets, plan.data(), 0, rgb->data(), status);
    if (g_sync) {
      std::vector<uint8_t> again(rgb->size(), 0);
      int32_t st = -1;
      if (jpgd_build_plan(exact, offsets, 1, plan.data(), plan.size(), err, sizeof(err), g_entropy, g_sync)) st = -2;
      else jpgd_host_frame(exact, offsets, plan.data(), 0, again.data(), &st);
      g_sync_differs += st != *status || again != *rgb;
    }
  }
  *why = err;
  free(exact);
  return rc;
}

// ---------------------------------------------------------------- --selftest: headers no encoder writes, built here
// An 8 x 8 grey file whose two Huffman tables hold one 1-bit code each (DC category 0, AC end-of-block): the scan is the byte
// 0x3F and every pixel is 128.  The variants change one thing in the header each.
struct Crafted {
  const char* name;
  bool refused;  // what the plan must do
  std::vector<uint8_t> bytes;
};
static void put(std::vector<uint8_t>& v, std::initializer_list<int> b) {
  for (int x : b) v.push_back((uint8_t)x);
}
static void put_dht(std::vector<uint8_t>& v, int tc_th, int first_bits, int n_vals) {  // the table alone, no marker
  v.push_back((uint8_t)tc_th), v.push_back((uint8_t)first_bits);
  for (int i = 1; i < 16; ++i) v.push_back(0);
  for (int i = 0; i < n_vals; ++i) v.push_back(0);
}
enum { kPlain, kDhtThree, kDhtTwoHundred, kDhtTooMany, kDhtJoined, kDqt16, kDriBeyond };
static std::vector<uint8_t> craft(int what) {
  std::vector<uint8_t> v;
  put(v, {0xFF, 0xD8});
  if (what == kDqt16) {
    put(v, {0xFF, 0xDB, 0, 131, 0x10});
    for (int i = 0; i < 64; ++i) put(v, {i == 0 ? 1 : 0, i == 0 ? 44 : 1});  // 300 at DC: a 16-bit entry
  } else {
    put(v, {0xFF, 0xDB, 0, 67, 0});
    for (int i = 0; i < 64; ++i) v.push_back(1);
  }
  put(v, {0xFF, 0xC0, 0, 11, 8, 0, 8, 0, 8, 1, 1, 0x11, 0});
  if (what == kDhtJoined) {  // both tables in one segment
    put(v, {0xFF, 0xC4, 0, 2 + 2 * 18});
    put_dht(v, 0x00, 1, 1), put_dht(v, 0x10, 1, 1);
  } else {
    const int n = what == kDhtThree ? 3 : what == kDhtTwoHundred ? 200 : 1;  // codes of length 1: two exist
    put(v, {0xFF, 0xC4, 0, 19 + n});
    put_dht(v, 0x00, n, n);
    if (what == kDhtTooMany) {  // lengths that fit (2 of 15 bits, 255 of 16) but 257 values
      put(v, {0xFF, 0xC4, 1, 20, 0x10});
      for (int i = 0; i < 16; ++i) v.push_back(i == 14 ? 2 : i == 15 ? 255 : 0);
      for (int i = 0; i < 257; ++i) v.push_back(0);
    } else {
      put(v, {0xFF, 0xC4, 0, 20});
      put_dht(v, 0x10, 1, 1);
    }
  }
  if (what == kDriBeyond) put(v, {0xFF, 0xDD, 0, 4, 0, 5});  // 5 MCUs per interval, the frame has 1
  put(v, {0xFF, 0xDA, 0, 8, 1, 1, 0x00, 0, 63, 0, 0x3F, 0xFF, 0xD9});
  return v;
}
static int selftest() {
  const Crafted cases[] = {{"plain", false, craft(kPlain)},
                           {"DHT with 3 codes of length 1", true, craft(kDhtThree)},
                           {"DHT with 200 codes of length 1", true, craft(kDhtTwoHundred)},
                           {"DHT with 257 values", true, craft(kDhtTooMany)},
                           {"two tables in one DHT segment", false, craft(kDhtJoined)},
                           {"16-bit DQT", false, craft(kDqt16)},
                           {"DRI beyond the frame's MCUs", false, craft(kDriBeyond)}};
  int bad = 0;
  for (const Crafted& c : cases) {
    std::vector<uint8_t> rgb;
    std::string why;
    int32_t st = -1;
    const bool refused = decode(c.bytes.data(), c.bytes.size(), &rgb, &st, &why) != 0;
    bool ok = refused == c.refused;
    if (ok && !refused) {
      ok = st == 0 && rgb.size() == 192;
      for (uint8_t p : rgb) ok = ok && p == 128;
    }
    printf("selftest %-34s %s%s%s\n", c.name, ok ? "ok" : "WRONG", refused ? ": refused: " : "", why.c_str());
    bad += !ok;
  }
  return bad;
}

int main(int argc, char** argv) {
  bool mangle = false;
  int files = 0, refused = 0, flagged = 0, clean = 0, wrong = 0;
  for (int a = 1; a < argc; ++a) {
    if (std::string(argv[a]) == "--selftest") {
      wrong += selftest();
      continue;
    }
    if (std::string(argv[a]) == "--mangle") {
      mangle = true;
      continue;
    }
    if ((std::string(argv[a]) == "--sync" || std::string(argv[a]) == "--split") && a + 1 < argc) {
      g_entropy = std::string(argv[a]) == "--split" ? 3 : 1;
      g_sync = atoi(argv[++a]);
      continue;
    }
    const std::vector<uint8_t> src = slurp(argv[a]);
    std::vector<uint8_t> rgb;
    std::string why;
    int32_t st = 0;
    ++files;
    if (decode(src.data(), src.size(), &rgb, &st, &why)) {
      printf("%s: refused: %s\n", argv[a], why.c_str());
      ++refused;
      continue;
    }
    const std::vector<uint8_t> want = slurp(std::string(argv[a]).substr(0, std::string(argv[a]).rfind('.')) + ".rgb");
    if (!want.empty() && want != rgb) printf("%s: differs from its .rgb\n", argv[a]), ++wrong;
    if (st) printf("%s: status %d\n", argv[a], st);
    if (!mangle) continue;
    uint32_t rng = 12345u + (uint32_t)src.size();
    auto next = [&rng]() { return rng = rng * 1664525u + 1013904223u; };
    for (int i = 0; i < 64 + 256; ++i) {
      std::vector<uint8_t> v = src;
      if (i < 64) v.resize(next() % src.size());
      else v[next() % src.size()] ^= (uint8_t)(1u << (next() >> 29));
      if (decode(v.data(), v.size(), &rgb, &st, &why)) ++refused;
      else (st ? flagged : clean)++;
    }
  }
  printf("%d files; mangled copies: %d refused, %d decoded with a status, %d decoded clean; %d differ from their .rgb\n", files, refused, flagged,
         clean, wrong);
  if (g_sync) printf("%s %d: %d decodes differ from the interval route\n", g_entropy == 3 ? "--split" : "--sync", g_sync, g_sync_differs);
  return wrong || g_sync_differs ? 1 : 0;
}
