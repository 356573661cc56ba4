// dtk_model.cpp -- host side of libdatok_gpu.so: the error state, the device entry points, the test hooks, and the
// model files (.matok / .datok, and Foma text nets through dtk_foma.cpp) with their device tables.  Everything that
// computes runs in the .hip units (symbolize, walk, repair, compact, render); nothing here walks the automaton.
#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "dtk_host.h"

// --------------------------------------------------------------- error state

static thread_local std::string g_hip_err;

int hip_fail(hipError_t e, const char *what) {
  g_hip_err = std::string(what) + ": " + hipGetErrorString(e);
  return e == hipErrorNoDevice || e == hipErrorInvalidDevice ? DTK_E_NO_DEVICE : DTK_E_HIP;
}

extern "C" const char *dtk_last_hip_error(void) { return g_hip_err.c_str(); }

extern "C" const char *dtk_strerror(int code) {
  switch (code) {
    case DTK_OK: return "ok";
    case DTK_E_IO: return "cannot open or read the tokenizer file";
    case DTK_E_FORMAT: return "not a gzip'd MATOK/DATOK file (magic, version or length)";
    case DTK_E_NO_DEVICE: return "no usable HIP device (this library has no CPU path)";
    case DTK_E_HIP: return "HIP runtime error (see dtk_last_hip_error)";
    case DTK_E_ARG: return "invalid argument";
    case DTK_E_MODEL: return "model outside device limits (symbols >= 2048, special ids out of range, epsilon cycle)";
    case DTK_E_CAPACITY: return "batch exceeds the capacity it was created with";
    case DTK_E_STATE: return "call out of order";
    case DTK_E_NOMEM: return "out of host memory";
    case DTK_E_IRREGULAR: return "a slice of the stream needs the exact pass: tokenize the text as one document";
    default: return "unknown error";
  }
}

extern "C" int dtk_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

extern "C" int dtk_set_device(int device) {
  HIP_TRY(hipSetDevice(device));
  return DTK_OK;
}

DtkDebug g_dbg;  // (test hooks, dtk_host.h)

extern "C" int dtk_debug_configure(const char *key, const char *value) {
  if (!key) return DTK_E_ARG;
  const int v = value ? atoi(value) : 1;
  const struct { const char *name; int *field; bool flag; } tab[] = {
      {"SYM16", &g_dbg.sym16, true}, {"GENERAL16", &g_dbg.general16, true}, {"FORCE_WIDE", &g_dbg.force_wide, true}, {"FILE_COLUMNS", &g_dbg.file_columns, true},
      {"NO_FUSED", &g_dbg.no_fused, true}, {"WIDE_FUSED", &g_dbg.wide_fused, true}, {"NO_DENSE", &g_dbg.no_dense, true}, {"SMALL_MAX", &g_dbg.small_max, false},
      {"LDS_BITS", &g_dbg.lds_bits, false}, {"SPLIT_START", &g_dbg.split_start, false}, {"DEV_ROUNDS", &g_dbg.dev_rounds, false},
      {"COMPACT_FULL", &g_dbg.compact_full, true}, {"CLEAR_KERNEL", &g_dbg.clear_kernel, true},
      {"ROUND_LIMIT", &g_dbg.round_limit, false}, {"DEBUG_REPAIR", &g_dbg.debug_repair, true},
      {"BLK_SPAN", &g_dbg.blk_span, false}, {"EVL_CAP", &g_dbg.evl_cap, false},
      {"SEN_CAP", &g_dbg.sen_cap, false}, {"VOCAB_HASH_BITS", &g_dbg.vocab_hash_bits, false}};
  if (strncmp(key, "DATOK_", 6) == 0) key += 6;
  if (strcmp(key, "SP_POSC0") == 0) {  // (a 64-bit value)
    g_dbg.sp_posc0 = value ? atoll(value) : 0;
    return DTK_OK;
  }
  for (const auto &e : tab)
    if (strcmp(key, e.name) == 0) {
      // (a flag is on by being named, as the environment variables were: `DATOK_NO_FUSED=` or `=1` both switch it on)
      *e.field = e.flag ? ((value && value[0] == '0' && value[1] == 0) ? 0 : 1) : v;
      return DTK_OK;
    }
  return DTK_E_ARG;
}

// ------------------------------------------------------------------- model

// Go unicode/utf8.DecodeRune (host copy, used for the sigma block of the model
// files, matrix.go:296 / datok.go:687, and for rendering surfaces).
int go_decode_host(const uint8_t *p, size_t n, uint32_t *r) {
  *r = 0xFFFD;
  if (n == 0) return 0;
  uint32_t b0 = p[0];
  if (b0 < 0x80) { *r = b0; return 1; }
  if (b0 < 0xC2 || b0 > 0xF4) return 1;
  if (b0 < 0xE0) {
    if (n < 2 || (p[1] & 0xC0) != 0x80) return 1;
    *r = ((b0 & 0x1F) << 6) | (p[1] & 0x3F);
    return 2;
  }
  if (b0 < 0xF0) {
    uint32_t lo = b0 == 0xE0 ? 0xA0 : 0x80, hi = b0 == 0xED ? 0x9F : 0xBF;
    if (n < 3 || p[1] < lo || p[1] > hi || (p[2] & 0xC0) != 0x80) return 1;
    *r = ((b0 & 0x0F) << 12) | ((uint32_t)(p[1] & 0x3F) << 6) | (p[2] & 0x3F);
    return 3;
  }
  uint32_t lo = b0 == 0xF0 ? 0x90 : 0x80, hi = b0 == 0xF4 ? 0x8F : 0xBF;
  if (n < 4 || p[1] < lo || p[1] > hi || (p[2] & 0xC0) != 0x80 || (p[3] & 0xC0) != 0x80) return 1;
  *r = ((b0 & 0x07) << 18) | ((uint32_t)(p[1] & 0x3F) << 12) | ((uint32_t)(p[2] & 0x3F) << 6) | (p[3] & 0x3F);
  return 4;
}

static uint16_t rd16(const uint8_t *p) { return (uint16_t)(p[0] | (p[1] << 8)); }
static uint32_t rd32(const uint8_t *p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// gzip.NewReader + ReadAll (matrix.go:222, fomafile.go:460)
int gunzip(const uint8_t *gz, size_t n, std::vector<uint8_t> &out) {
  if (n < 18 || gz[0] != 0x1f || gz[1] != 0x8b) return DTK_E_FORMAT;
  z_stream zs;
  memset(&zs, 0, sizeof zs);
  if (inflateInit2(&zs, 16 + MAX_WBITS) != Z_OK) return DTK_E_FORMAT;
  zs.next_in = const_cast<Bytef *>(gz);
  zs.avail_in = (uInt)n;
  out.resize(std::max<size_t>(n * 8, 1 << 16));
  size_t have = 0;
  int rc;
  do {
    if (have == out.size()) out.resize(out.size() * 2);
    zs.next_out = out.data() + have;
    zs.avail_out = (uInt)std::min<size_t>(out.size() - have, 1u << 30);
    const size_t before = zs.avail_out;
    rc = inflate(&zs, Z_NO_FLUSH);
    have += before - zs.avail_out;
  } while (rc == Z_OK);
  inflateEnd(&zs);
  if (rc != Z_STREAM_END) return DTK_E_FORMAT;
  out.resize(have);
  return DTK_OK;
}

// Sigma block: sigmaCount UTF-8 runes, NUL = "no character" (matrix.go:288-303,
// datok.go:679-694).  A later index overwrites an earlier one, like the Go map.
static size_t parse_sigma(dtk_model *m, const std::vector<uint8_t> &raw, size_t off) {
  for (int i = 0; i < 256; i++) m->ascii[i] = (uint16_t)m->identity;
  std::vector<std::pair<uint32_t, uint16_t>> ent;
  for (int x = 0; x < m->sigma_count; x++) {
    if (off >= raw.size()) continue;
    uint32_t r;
    int w = go_decode_host(raw.data() + off, raw.size() - off, &r);
    off += (size_t)w;
    if (r != 0) {
      if (r < 256) m->ascii[r] = (uint16_t)x;
      ent.emplace_back(r, (uint16_t)x);
    }
  }
  std::stable_sort(ent.begin(), ent.end(),
                   [](const auto &a, const auto &b) { return a.first < b.first; });
  for (auto &e : ent) {
    if (!m->sigma_runes.empty() && m->sigma_runes.back() == e.first) m->sigma_syms.back() = e.second;
    else { m->sigma_runes.push_back(e.first); m->sigma_syms.push_back(e.second); }
  }
  return off;
}

// What upload() brings to the device besides the table: built on the host first (build_images), so that
// dtk_model_info_mem can answer for a model without a device.
struct HostImages {
  size_t slack = 0;                 // zeroed bytes behind the table
  uint16_t ascii_dev[256];
  size_t first = 0, nr = 0;         // the sigma runes >= 256: sigma_runes[first .. first + nr)
  std::vector<uint16_t> syms_dev;   // their columns
  std::vector<uint16_t> entries;    // code -> stream entry [256]
  std::vector<uint8_t> bytes;       // rune < 256 -> code [256], sigma rune >= 256 -> code [nr]
};

// symbols as the device sees them: the column of the table they index, see layout_matrix
static uint32_t colof(const dtk_model *m, int sym) {
  return (sym >= 0 && (size_t)sym < m->col.size()) ? m->col[(size_t)sym] : (uint32_t)sym;
}

// Everything about the device form of a model that is decided on the host: the symbol tables, the stream's code
// table, the special symbols as columns, and what the model will hold in HBM.
static void build_images(dtk_model *m, size_t tab_bytes, HostImages &im) {
  // (2048 cells of slack behind the last row: the lean walk asks for its next cell before it knows that the reader is
  //  at EOF, with whatever stream entry lies behind the document -- any 11-bit symbol index; the cell is not used)
  const bool cells64 = m->tab.kind == DTK_KIND_MATRIX && m->tab.fused && m->tab.entry_bytes == 8;
  im.slack = (DTK_SYM_MASK + 1u) * (cells64 ? 8u : 4u);
  for (int i = 0; i < 256; i++) im.ascii_dev[i] = (uint16_t)colof(m, m->ascii[i]);
  // the device's sorted rune list only holds runes >= 256 (the others go through the 256-entry table)
  size_t first = 0;
  while (first < m->sigma_runes.size() && m->sigma_runes[first] < 256u) first++;
  const size_t nr = m->sigma_runes.size() - first;
  im.first = first; im.nr = nr;
  im.syms_dev.resize(nr);
  for (size_t i = 0; i < nr; i++) im.syms_dev[i] = (uint16_t)colof(m, m->sigma_syms[first + i]);
  m->device_bytes = tab_bytes + im.slack + 512 + nr * 6;
  {
    // The stream's code table (dtk_internal.h): every entry the symboliser can write for this model, numbered.
    std::vector<uint16_t> &entries = im.entries;
    bool fits = true;
    auto code_of = [&](uint32_t e) -> uint8_t {
      for (size_t i = 0; i < entries.size(); i++)
        if (entries[i] == (uint16_t)e) return (uint8_t)i;
      if (entries.size() >= DTK_SYM_CONT) { fits = false; return 0; }
      entries.push_back((uint16_t)e);
      return (uint8_t)(entries.size() - 1);
    };
    const uint32_t ident = m->identity < 0 ? 0u : colof(m, m->identity);
    std::vector<uint8_t> &bytes = im.bytes;
    bytes.assign(256 + nr, 0);
    for (uint32_t i = 0; i < 256; i++) {  // matrix.go:421-426; a rune of 128..255 takes two bytes
      const uint32_t e = (im.ascii_dev[i] & DTK_SYM_MASK) | (i == DTK_EOT ? 1u << DTK_SYM_CLS_SHIFT : 0u) |
                         ((i < 128 ? 1u : 2u) << DTK_SYM_W_SHIFT);
      // (the code of a byte < 128 is the byte: the symboliser copies those, k_symbolize's light path)
      if (i < 128) { entries.push_back((uint16_t)e); bytes[i] = (uint8_t)i; } else bytes[i] = code_of(e);
    }
    uint32_t fffd = (ident & DTK_SYM_MASK) | (3u << DTK_SYM_CLS_SHIFT);
    for (size_t i = 0; i < nr; i++) {
      const uint32_t r = m->sigma_runes[first + i], w = r < 0x800u ? 2u : (r < 0x10000u ? 3u : 4u);
      const uint32_t e = (colof(m, m->sigma_syms[first + i]) & DTK_SYM_MASK) | (2u << DTK_SYM_CLS_SHIFT);
      bytes[256 + i] = code_of(e | (w << DTK_SYM_W_SHIFT));
      if (r == 0xFFFDu) fffd = e;
    }
    for (uint32_t w = 1; w <= 4; w++)
      m->sig.code_ident[w] = code_of((ident & DTK_SYM_MASK) | (3u << DTK_SYM_CLS_SHIFT) | (w << DTK_SYM_W_SHIFT));
    m->sig.code_ident[0] = DTK_SYM_CONT;
    m->sig.code_fffd1 = code_of(fffd | (1u << DTK_SYM_W_SHIFT));  // an invalid byte decodes to U+FFFD, one byte wide
    m->sig.n_codes = (fits && !g_dbg.sym16) ? (uint32_t)entries.size() : 0u;
    entries.resize(256, 0);  // (DTK_SYM_CONT and the unused codes: width 0)
    m->device_bytes += 512 + bytes.size();
  }
  m->sig.n_runes = (uint32_t)nr;
  // a net without identity symbol (-1, fomafile.go:88): unmapped runes get symbol 0, which has
  // no arcs (matrix.go:459), and no symbol ever equals the identity (matrix.go:478)
  m->sig.identity = m->identity < 0 ? 0u : colof(m, m->identity);
  m->tab.epsilon = colof(m, m->epsilon);
  m->tab.unknown = m->unknown < 0 ? (uint32_t)m->unknown : colof(m, m->unknown);
  m->tab.identity = m->identity < 0 ? (uint32_t)m->identity : colof(m, m->identity);
  if (m->tab.ident_guard != 0xFFFFFFFFu) m->tab.ident_guard = colof(m, (int)m->tab.ident_guard);
  // Which loop (with_trans, dtk_walk_core.h): the lean one for fused cells without an arc on `unknown`, over codes
  // or over 16-bit entries alike.
  m->tab.lean16 = g_dbg.general16 ? 0u : 1u;
  m->lean_walk = (m->tab.kind == DTK_KIND_MATRIX && m->tab.fused && m->tab.ident_guard == 0xFFFFFFFFu &&
                  (m->sig.n_codes != 0 || m->tab.lean16)) ? 1u : 0u;
}

static int copy_images(dtk_model *m, const void *tab, size_t tab_bytes, const HostImages &im) {
  HIP_TRY(hipGetDevice(&m->device));
  auto make = [](auto &a, size_t n) { return a.fit(n, n); };
  int rc;
  if ((rc = make(m->d_tab, std::max<size_t>(tab_bytes, 16) + im.slack))) return rc;
  HIP_TRY(hipMemset(m->d_tab + tab_bytes, 0, im.slack));
  HIP_TRY(hipMemcpy(m->d_tab, tab, tab_bytes, hipMemcpyHostToDevice));
  if ((rc = make(m->d_ascii, 256))) return rc;
  HIP_TRY(hipMemcpy(m->d_ascii, im.ascii_dev, 256 * sizeof(uint16_t), hipMemcpyHostToDevice));
  const size_t nr = im.nr;
  if ((rc = make(m->d_runes, std::max<size_t>(nr, 1))) || (rc = make(m->d_syms, std::max<size_t>(nr, 1)))) return rc;
  if (nr) {
    HIP_TRY(hipMemcpy(m->d_runes, m->sigma_runes.data() + im.first, nr * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m->d_syms, im.syms_dev.data(), nr * sizeof(uint16_t), hipMemcpyHostToDevice));
  }
  if ((rc = make(m->d_codes, 512 + im.bytes.size()))) return rc;
  HIP_TRY(hipMemcpy(m->d_codes, im.entries.data(), 512, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(m->d_codes + 512, im.bytes.data(), im.bytes.size(), hipMemcpyHostToDevice));
  m->sig.code_entry = (const uint16_t *)m->d_codes.p;
  m->sig.code_lt256 = m->d_codes + 512;
  m->sig.code_runes = m->d_codes + 768;
  m->sig.ascii = m->d_ascii;
  m->sig.runes = m->d_runes;
  m->sig.syms = m->d_syms;
  m->tab.tab = m->d_tab;
  return DTK_OK;
}

// the device form of a model whose table image is `tab`: built on the host, then copied (unless nobody asked for a device)
static int upload(dtk_model *m, const void *tab, size_t tab_bytes) {
  HostImages im;
  build_images(m, tab_bytes, im);
  return m->host_only ? DTK_OK : copy_images(m, tab, tab_bytes, im);
}

bool special_ids_ok(const dtk_model *m) {
  // The walk compares symbols against these ids; the symbol stream has 11 bits.
  // identity == unknown makes the retry of matrix.go:478-485 spin forever upstream.
  return m->sigma_count >= 1 && m->sigma_count <= (int)DTK_SYM_MAX && m->epsilon >= 1 &&
         m->epsilon < m->sigma_count && m->unknown < m->sigma_count && m->identity < m->sigma_count &&
         (m->identity != m->unknown || m->identity < 0) && m->epsilon != m->identity;
}


// The cell encoding of a matrix table with states 1..N and S symbols (layout_matrix; build_datok asks before it
// densifies a double array).
//   FUSED32  15-bit state ids: target | nontoken<<15 | via<<16 | fused<<31 in one uint32
//   FUSED64  larger automata: uint2, .x = target[29:0] | nontoken<<30 | fused<<31, .y = via.  The lean loop addresses a
//            cell by a 32-bit BYTE offset that it gets from one 24-bit multiply-add (DTK_TAB, dtk_walk_core.h), so this
//            form applies when   N + 1 < 2^24   and   ((N + 1) * stride + 2048) * 8 < 2^32   (2048: the slack cells)
//   PLAIN16 / PLAIN32  target | nontoken in the top bit, no fused cells: what DATOK_NO_FUSED / DATOK_FORCE_WIDE select
//            for the tests, and what a table beyond the 32-bit byte offset keeps
enum CellEnc { ENC_PLAIN16, ENC_PLAIN32, ENC_FUSED32, ENC_FUSED64 };
static uint32_t stride_of(uint64_t S) { return (uint32_t)((S + 7) & ~7ull); }
static CellEnc pick_encoding(uint64_t N, uint64_t S) {
  const bool fits15 = (N + 1) <= 0x7FFFu;
  if (g_dbg.force_wide) return ENC_PLAIN32;
  if (g_dbg.no_fused) return fits15 ? ENC_PLAIN16 : ENC_PLAIN32;
  if (fits15 && !g_dbg.wide_fused) return ENC_FUSED32;
  const bool fits64 = (N + 1) < (1ull << 24) && ((N + 1) * stride_of(S) + (DTK_SYM_MASK + 1u)) * 8ull < (1ull << 32);
  if (fits64) return ENC_FUSED64;
  return fits15 ? ENC_FUSED32 : ENC_PLAIN32;
}

// ParseMatrix (matrix.go:235-337)
static int build_matrix(dtk_model *m, const std::vector<uint8_t> &raw) {
  if (raw.size() < 19) return DTK_E_FORMAT;
  const uint8_t *h = raw.data() + 5;
  if (rd16(h) != 1) return DTK_E_FORMAT;  // VERSION
  m->kind = DTK_KIND_MATRIX;
  m->epsilon = rd16(h + 2);
  m->unknown = rd16(h + 4);
  m->identity = rd16(h + 6);
  m->state_count = rd32(h + 8);
  m->sigma_count = rd16(h + 12);
  m->array_len = ((uint64_t)m->state_count + 1) * (uint64_t)m->sigma_count;  // matrix.go:286
  size_t off = parse_sigma(m, raw, 19);
  if (off >= raw.size() || raw[off] != 'M') return DTK_E_FORMAT;  // matrix.go:305-315
  off++;
  if (raw.size() - off < m->array_len * 4) return DTK_E_FORMAT;   // matrix.go:327-330
  if (!special_ids_ok(m) || m->state_count == 0 || m->state_count >= 0x7FFFFFFFu) return DTK_E_MODEL;
  std::vector<uint32_t> arr(m->array_len);
  for (uint64_t x = 0; x < m->array_len; x++) arr[x] = rd32(raw.data() + off + x * 4);
  return layout_matrix(m, arr, m->state_count, false);
}

// Device layout of a matrix tokenizer whose header fields and sigma are set in `m` and whose
// symbol-major array (matrix.go:463) is `arr`.
// (n_states / da_dense: the same layout for the transitions of a double-array tokenizer, see densify_datok)
int layout_matrix(dtk_model *m, const std::vector<uint32_t> &arr, uint64_t n_states, bool da_dense) {
  const uint64_t N = n_states, S = (uint64_t)m->sigma_count;
  auto cell = [&](uint64_t a, uint64_t t) -> uint32_t {  // array[(a-1)*stateCount + t], matrix.go:463
    return arr[(a - 1) * N + t];
  };

  // renumber: states with an epsilon arc first (probe of matrix.go:442 -> compare)
  std::vector<uint32_t> newid(N + 1, 0);
  uint32_t next = 1;
  for (uint64_t t = 1; t <= N; t++)
    if (cell((uint64_t)m->epsilon, t) != 0) newid[t] = next++;
  m->n_eps_states = next - 1;
  for (uint64_t t = 1; t <= N; t++)
    if (newid[t] == 0) newid[t] = next++;

  // epsilon chains: reject cycles (the reference would never return, matrix.go:633-634)
  {
    std::vector<uint32_t> depth(N + 1, 0);
    uint32_t best = 0;
    for (uint64_t t = 1; t <= N; t++) {
      uint64_t cur = t;
      uint32_t len = 0;
      while (true) {
        uint32_t nx = cell((uint64_t)m->epsilon, cur) & ~DTK_FIRSTBIT;
        if (nx == 0 || nx > N) break;
        len++;
        if (len > N) return DTK_E_MODEL;
        cur = nx;
      }
      best = std::max(best, len);
    }
    m->max_eps_chain = best;
  }

  // the cell encoding: fused cells of 32 bits where the state ids fit 15, of 64 bits beyond (pick_encoding)
  const CellEnc enc = pick_encoding(N, S);
  const uint32_t stride = stride_of(S);
  const size_t cells_total = (size_t)(N + 1) * stride;
  // Columns: the symbols of running text first -- blank, the lower-case letters by frequency, full stop, comma,
  // newline, umlauts, digits, capitals --, so that the cells a row is mostly asked for share one or two cache lines
  // (in file order the letters, the blank and the punctuation of a row lie in four or five).  Symbol 0 keeps
  // column 0 (no arcs, matrix.go:459).  The device's symbol tables and special symbols are mapped in upload().
  std::vector<uint16_t> &col = m->col;
  col.assign((size_t)S, 0xFFFFu);
  {
    static const uint32_t order[] = {' ', 'e', 'n', 'i', 's', 'r', 'a', 't', 'd', 'h', 'u', 'l', 'c', 'g', 'm', 'o', 'b', 'w', 'f',
                                     'k', 'z', 'p', 'v', '.', ',', '\n', 0xFC, 0xE4, 0xF6, 0xDF, 'j', 'y', 'x', 'q', '-', '\'', '"',
                                     '0', '1', '2', '3', '4', '5', '6', '7', '8', '9', 'S', 'D', 'A', 'E', 'B', 'M', 'K', 'W', 'G',
                                     'H', 'T', 'I', 'P', 'L', 'R', 'F', 'N', 'V', 'Z', 'U', 'O', 'J', 'C', ':', ';', '?', '!', '(', ')',
                                     '/', '\t', '\r'};
    uint32_t next_col = 1;
    col[0] = 0;
    if (!g_dbg.file_columns)
      for (uint32_t r : order)
        for (size_t i = 0; i < m->sigma_runes.size(); i++)
          if (m->sigma_runes[i] == r) {
            const uint32_t a = m->sigma_syms[i];
            if (a > 0 && a < S && col[a] == 0xFFFFu) col[a] = (uint16_t)next_col++;
          }
    for (uint64_t a = 1; a < S; a++)
      if (col[a] == 0xFFFFu) col[a] = (uint16_t)next_col++;
  }
  const bool fused = enc == ENC_FUSED32 || enc == ENC_FUSED64;
  const size_t cell_bytes = enc == ENC_FUSED64 ? 8 : (enc == ENC_PLAIN16 ? 2 : 4);
  std::vector<uint8_t> host(cells_total * cell_bytes, 0);
  // a cell: target, nontoken flag, and for a fused cell the epsilon target it goes through (else via = 0)
  auto put = [&](size_t at, uint32_t tgt, bool nontoken, uint32_t via) {
    switch (enc) {
      case ENC_FUSED64: {
        const uint32_t v[2] = {tgt | (nontoken ? 0x40000000u : 0u) | (via ? 0x80000000u : 0u), via};
        memcpy(host.data() + at * 8, v, 8);
        break;
      }
      case ENC_FUSED32: {
        const uint32_t v = tgt | (nontoken ? 0x8000u : 0u) | (via ? 0x80000000u | (via << 16) : 0u);
        memcpy(host.data() + at * 4, &v, 4);
        break;
      }
      case ENC_PLAIN32: {
        const uint32_t v = tgt | (nontoken ? DTK_FIRSTBIT : 0u);
        memcpy(host.data() + at * 4, &v, 4);
        break;
      }
      case ENC_PLAIN16: {
        const uint16_t h = (uint16_t)(tgt | (nontoken ? 0x8000u : 0u));
        memcpy(host.data() + at * 2, &h, 2);
        break;
      }
    }
  };
  for (uint64_t a = 1; a < S; a++) {
    for (uint64_t t = 1; t <= N; t++) {
      const uint32_t x = cell(a, t);
      const uint32_t tgt = x & ~DTK_FIRSTBIT;
      if (tgt == 0) continue;
      if (tgt > N) return DTK_E_MODEL;
      if ((int)a == m->unknown) m->unknown_used = 1;
      put((size_t)newid[t] * stride + col[a], newid[tgt], (x & DTK_FIRSTBIT) != 0, 0u);
    }
  }
  if (fused) {
    // (t, a) empty, t --epsilon--> e, (e, a) present: the fused cell  cell(e, a) through e
    for (uint64_t t = 1; t <= N; t++) {
      const uint32_t e = cell((uint64_t)m->epsilon, t) & ~DTK_FIRSTBIT;
      if (e == 0 || e > N) continue;
      for (uint64_t a = 1; a < S; a++) {
        if ((int)a == m->epsilon || (int)a == m->unknown) continue;
        if ((cell(a, t) & ~DTK_FIRSTBIT) != 0) continue;
        const uint32_t x2 = cell(a, e);
        const uint32_t tgt2 = x2 & ~DTK_FIRSTBIT;
        if (tgt2 == 0 || tgt2 > N) continue;
        put((size_t)newid[t] * stride + col[a], newid[tgt2], (x2 & DTK_FIRSTBIT) != 0, newid[e]);
      }
    }
  }
  m->tab.kind = DTK_KIND_MATRIX;
  m->tab.entry_bytes = (uint32_t)cell_bytes;
  m->tab.fused = fused ? 1u : 0u;
  m->tab.ident_guard = m->unknown_used ? (uint32_t)m->identity : 0xFFFFFFFFu;
  m->tab.da_dense = da_dense ? 1u : 0u;
  m->tab.stride = stride;
  m->tab.n_states = (uint32_t)N;
  m->tab.n_eps = m->n_eps_states;
  m->tab.start = newid[1];
  return upload(m, host.data(), host.size());
}

// ParseDatok (datok.go:621-729) + device layout.
static int build_datok(dtk_model *m, const std::vector<uint8_t> &raw) {
  if (raw.size() < 21) return DTK_E_FORMAT;
  const uint8_t *h = raw.data() + 5;
  if (rd16(h) != 1) return DTK_E_FORMAT;
  m->kind = DTK_KIND_DA;
  m->epsilon = rd16(h + 2);
  m->unknown = rd16(h + 4);
  m->identity = rd16(h + 6);
  m->final_state = rd16(h + 8);
  m->sigma_count = rd16(h + 10);
  m->array_len = rd32(h + 12) / 2;  // "Legacy support", datok.go:674
  size_t off = parse_sigma(m, raw, 21);
  if (off >= raw.size() || raw[off] != 'T') return DTK_E_FORMAT;
  off++;
  if (raw.size() - off < m->array_len * 8) return DTK_E_FORMAT;
  if (!special_ids_ok(m) || m->array_len < 2 || m->array_len >= DTK_RESTBIT) return DTK_E_MODEL;

  const uint64_t L = m->array_len;
  std::vector<uint32_t> bc(L * 2);
  for (uint64_t i = 0; i < L * 2; i++) bc[i] = rd32(raw.data() + off + i * 4);
  const uint32_t size = bc[3] & DTK_RESTBIT;  // array[1].check, datok.go:333-335
  m->state_count = size;
  auto has_eps = [&](uint64_t s) -> bool {  // datok.go:876
    const uint64_t ei = (uint64_t)(bc[2 * s] & DTK_RESTBIT) + (uint32_t)m->epsilon;
    return ei < L && (bc[2 * ei + 1] & DTK_RESTBIT) == s;
  };
  // epsilon arc target incl. representative hop (datok.go:889-901, 1056-1058)
  auto eps_target = [&](uint64_t s) -> uint64_t {
    const uint64_t ei = (uint64_t)(bc[2 * s] & DTK_RESTBIT) + (uint32_t)m->epsilon;
    if (ei >= L || ei > size || (bc[2 * ei + 1] & DTK_RESTBIT) != s) return 0;
    if (bc[2 * ei] & DTK_FIRSTBIT) return bc[2 * ei] & DTK_RESTBIT;
    return ei;
  };
  uint32_t neps = 0, best = 0;
  for (uint64_t s = 1; s < L; s++) {
    if (!has_eps(s)) continue;
    neps++;
    uint64_t cur = s;
    uint32_t len = 0;
    while (true) {
      uint64_t nx = eps_target(cur);
      if (nx == 0 || nx >= L) break;
      len++;
      if (len > 4096) return DTK_E_MODEL;  // epsilon cycle
      cur = nx;
    }
    best = std::max(best, len);
  }
  m->n_eps_states = neps;
  m->max_eps_chain = best;
  for (uint64_t i = 1; i < L && i <= size; i++) {
    const uint64_t par = bc[2 * i + 1] & DTK_RESTBIT;
    if (par && par < L && (uint64_t)(bc[2 * par] & DTK_RESTBIT) + (uint32_t)m->unknown == i) {
      m->unknown_used = 1;
      break;
    }
  }
  // The double array is a compressed encoding of the same kind of automaton the matrix holds dense: a shipped
  // model has some 20 000 states hidden in its 2.9 million pairs.  If they fit the fused cells (pick_encoding: 15-bit
  // state ids in 32-bit cells, 64-bit cells beyond), the device walks them as a matrix -- one load per step instead of
  // two dependent ones, the lean loop, fused epsilon cells -- under the double array's own rules for EOT
  // (datok.go:1019-1030; walk_fused<.., IS_MATRIX = false>, compaction and replay go by m->kind).  DATOK_NO_DENSE=1
  // keeps the pairs (DaTrans; what the tests of that path set).
  // (only with fused cells: the lean loop and the fused general loop carry the double array's EOT rules; the plain
  //  matrix encodings that DATOK_NO_FUSED / DATOK_FORCE_WIDE select for the tests are not run with them)
  if (!g_dbg.no_dense && !g_dbg.no_fused && !g_dbg.force_wide) {
    std::vector<uint32_t> arr;
    uint64_t n_dense = 0;
    // one step of datok.go:888-901 + 1055-1063 from state s0 on symbol a: 0 = no arc, else target | FIRSTBIT if
    // non-token; false = an access the reference would panic on (no dense form for such a file)
    auto step = [&](uint64_t s0, uint32_t a, uint32_t &out) -> bool {
      out = 0;
      const uint64_t idx = (uint64_t)(bc[2 * s0] & DTK_RESTBIT) + a;
      if (idx >= L) return false;          // datok.go:888-889 reads array[t] before any test: an index panic
      if (idx > size) {                    // datok.go:896: t > check(1) fails ...
        // ... but the epsilon probe of datok.go:876 has no such bound: a hand-made file whose state "has" an epsilon
        // arc behind check(1) remembers a slot the dense layout would not know -- the pairs are walked
        if (a == (uint32_t)m->epsilon && (bc[2 * idx + 1] & DTK_RESTBIT) == s0) return false;
        return true;
      }
      if ((bc[2 * idx + 1] & DTK_RESTBIT) != s0) return true;
      uint64_t t = idx;
      if (bc[2 * idx] & DTK_FIRSTBIT) {    // separate: the representative
        t = bc[2 * idx] & DTK_RESTBIT;
        if (t >= L || t == 0) return false;
      }
      out = (uint32_t)t | ((bc[2 * idx + 1] & DTK_FIRSTBIT) ? DTK_FIRSTBIT : 0u);
      return true;
    };
    bool ok = true;
    std::vector<uint32_t> id(L, 0);        // double-array index -> dense state number (1 = start)
    std::vector<uint64_t> order{0, 1};     // dense state number -> index
    id[1] = 1;
    const uint32_t S = (uint32_t)m->sigma_count;
    std::vector<uint32_t> trans;           // state-major while the states are being discovered
    for (uint64_t q = 1; ok && q < order.size(); q++) {
      const uint64_t s0 = order[q];
      uint32_t x;
      ok = step(s0, 0u, x) && x == 0u;     // symbol 0 must have no arc (the matrix's column 0, matrix.go:459)
      for (uint32_t a = 1; ok && a < S; a++) {
        ok = step(s0, a, x);
        const uint64_t t = x & ~DTK_FIRSTBIT;
        if (ok && t != 0 && id[t] == 0) {
          id[t] = (uint32_t)order.size();
          order.push_back(t);
          if (order.size() > 0x7FFFu) {    // (the 64-bit cells' limits only matter beyond the 15-bit ids)
            const CellEnc enc = pick_encoding(order.size() - 1, S);
            ok = enc == ENC_FUSED32 || enc == ENC_FUSED64;  // the fused cells must hold the reachable states
          }
        }
        trans.push_back(ok && t != 0 ? (id[t] | (x & DTK_FIRSTBIT)) : 0u);
      }
    }
    if (ok) {
      n_dense = order.size() - 1;
      arr.assign((size_t)(S - 1) * n_dense + n_dense + 1, 0);  // array[(a-1)*N + t], t in 1..N (matrix.go:463)
      for (uint64_t q = 1; q <= n_dense; q++)
        for (uint32_t a = 1; a < S; a++) arr[(size_t)(a - 1) * n_dense + q] = trans[(size_t)(q - 1) * (S - 1) + (a - 1)];
      const uint32_t keep_states = m->state_count;
      const int rc = layout_matrix(m, arr, n_dense, true);
      m->state_count = keep_states;
      m->dense_states = (uint32_t)n_dense;
      return rc;
    }
  }
  std::vector<uint32_t> dev(L * 2);
  for (uint64_t s = 0; s < L; s++) {
    dev[2 * s] = (bc[2 * s] & (DTK_FIRSTBIT | DTK_RESTBIT)) | (s >= 1 && has_eps(s) ? DTK_SECONDBIT : 0u);
    dev[2 * s + 1] = bc[2 * s + 1];
  }
  m->tab.kind = DTK_KIND_DA;
  m->tab.entry_bytes = 8;
  m->tab.da_len = (uint32_t)L;
  m->tab.da_size = size;
  m->tab.da_base1 = dev[2];
  m->tab.start = 1;
  return upload(m, dev.data(), dev.size() * 4);
}


// gunzip, sniff the magic (fomafile.go:476-482), parse, lay out: the device copy too unless m->host_only
static int build_model(dtk_model *m, const void *gz_bytes, size_t n) {
  std::vector<uint8_t> raw;
  int rc = gunzip((const uint8_t *)gz_bytes, n, raw);
  if (rc != DTK_OK) return rc;
  if (raw.size() < 5) return DTK_E_FORMAT;
  if (memcmp(raw.data(), "MATOK", 5) == 0) return build_matrix(m, raw);      // fomafile.go:476
  if (memcmp(raw.data(), "DATOK", 5) == 0) return build_datok(m, raw);       // fomafile.go:478
  if (raw.size() >= 10 && memcmp(raw.data(), "##foma-net", 10) == 0) return build_foma(m, raw);
  return DTK_E_FORMAT;                                                       // fomafile.go:482
}

extern "C" int dtk_model_load_mem(const void *gz_bytes, size_t n, dtk_model **out) {
  if (!gz_bytes || !out) return DTK_E_ARG;
  *out = nullptr;
  if (dtk_device_count() <= 0) return DTK_E_NO_DEVICE;
  dtk_model *m = new dtk_model();
  const int rc = build_model(m, gz_bytes, n);
  if (rc != DTK_OK) { delete m; return rc; }
  *out = m;
  return DTK_OK;
}

// Which path will this model take: the image is parsed and laid out exactly as dtk_model_load_mem does it, and
// nothing is copied anywhere.  Host only: needs no device.
extern "C" int dtk_model_info_mem(const void *gz_bytes, size_t n, dtk_model_info *out) {
  if (!gz_bytes || !out) return DTK_E_ARG;
  dtk_model m;
  m.host_only = true;
  const int rc = build_model(&m, gz_bytes, n);
  if (rc != DTK_OK) return rc;
  return dtk_model_get_info(&m, out);
}

extern "C" int dtk_model_load(const char *path, dtk_model **out) {
  if (!path || !out) return DTK_E_ARG;
  *out = nullptr;
  FILE *f = fopen(path, "rb");
  if (!f) return DTK_E_IO;
  std::vector<uint8_t> gz;
  uint8_t buf[1 << 16];
  size_t k;
  while ((k = fread(buf, 1, sizeof buf, f)) > 0) gz.insert(gz.end(), buf, buf + k);
  const bool bad = ferror(f) != 0;
  fclose(f);
  if (bad) return DTK_E_IO;
  return dtk_model_load_mem(gz.data(), gz.size(), out);
}

extern "C" void dtk_model_free(dtk_model *m) { delete m; }

extern "C" const char *dtk_model_type(const dtk_model *m) {
  return m->kind == DTK_KIND_MATRIX ? "MATOK" : "DATOK";
}

extern "C" int dtk_model_get_info(const dtk_model *m, dtk_model_info *o) {
  if (!m || !o) return DTK_E_ARG;
  o->kind = m->kind; o->epsilon = m->epsilon; o->unknown = m->unknown; o->identity = m->identity;
  o->final_state = m->final_state; o->sigma_count = m->sigma_count; o->state_count = m->state_count;
  o->array_len = m->array_len; o->n_eps_states = m->n_eps_states; o->max_eps_chain = m->max_eps_chain;
  o->entry_bytes = m->tab.entry_bytes; o->device_bytes = m->device_bytes; o->unknown_used = m->unknown_used;
  o->dense_states = m->dense_states;
  o->stream_codes = m->sig.n_codes;
  o->lean_walk = m->lean_walk;
  return DTK_OK;
}
