// engine_validate_host.cpp -- stand-alone host driver of csrc/engine_validate.h for tests/test_engine_file_cpu.py: the reading
// and validation steps of unina_load_engine's host side, built by a host compiler (no HIP, no GPU) and run over many damaged
// copies of one engine file.
//   engine_validate_host IN OUT
// IN : u64 magic "UNEVAL01", u64 base_len, the base engine file (base_len bytes), u64 n_cases, then per case
//      u32 case id, u32 n_edits, n_edits x (u64 offset, u32 width, u64 value): `value` is stored little endian over `width`
//      (1, 2, 4 or 8) bytes at `offset`, which must lie inside the header and the base file's two tables; width 0 is no store
//      but a truncation: the file ends after `value` bytes.
// OUT: per case (i32 case id, i32 code); stdout: a line "id code message" per case.
// Every case works on a fresh heap copy of the header and tables of exactly their size and reads the (never edited) blob bytes
// of the base only through the same bounds-checked reader, so a table entry read or an offset followed outside either is an
// error under -fsanitize=address, and arithmetic that wraps a signed value or shifts too far one under -fsanitize=undefined.
#include "../unina-yolo-dla_amd/csrc/engine_validate.h"

#include <cstdio>
#include <cstdlib>

using namespace unina;

namespace {
struct Cursor {
  const unsigned char* p;
  size_t left;
  template <class T> bool get(T* v) {
    if (left < sizeof(T)) return false;
    memcpy(v, p, sizeof(T));
    p += sizeof(T);
    left -= sizeof(T);
    return true;
  }
};
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  if (fseek(f, 0, SEEK_END)) return 3;
  const long in_len = ftell(f);
  if (in_len < 24 || fseek(f, 0, SEEK_SET)) return 3;
  unsigned char* in = (unsigned char*)malloc((size_t)in_len);
  if (!in || fread(in, 1, (size_t)in_len, f) != (size_t)in_len) return 3;
  fclose(f);
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 5;

  Cursor c{in, (size_t)in_len};
  uint64_t magic, base_len, n_cases;
  if (!c.get(&magic) || magic != 0x31304c4156454e55ull || !c.get(&base_len) || base_len > c.left) return 4;   // "UNEVAL01"
  const unsigned char* base = c.p;
  c.p += base_len;
  c.left -= base_len;
  if (!c.get(&n_cases)) return 4;
  // the editable prefix: the header and the tables as the BASE's header sizes them
  FileHeader bh;
  if (base_len < sizeof bh) return 4;
  memcpy(&bh, base, sizeof bh);
  if (!header_defect(bh).ok()) return 4;
  const uint64_t prefix = sizeof(FileHeader) + sizeof(BufferDesc) * (uint64_t)bh.n_buffers + sizeof(OpDesc) * (uint64_t)bh.n_ops;
  if (prefix > base_len) return 4;

  for (uint64_t k = 0; k < n_cases; ++k) {
    uint32_t id, n_edits;
    if (!c.get(&id) || !c.get(&n_edits)) return 4;
    unsigned char* head = (unsigned char*)malloc(prefix);
    if (!head) return 4;
    memcpy(head, base, prefix);
    uint64_t file_len = base_len;
    for (uint32_t e = 0; e < n_edits; ++e) {
      uint64_t off, value;
      uint32_t width;
      if (!c.get(&off) || !c.get(&width) || !c.get(&value)) return 4;
      if (width == 0) {
        if (value > base_len) return 4;
        file_len = value;
        continue;
      }
      if ((width != 1 && width != 2 && width != 4 && width != 8) || off > prefix || width > prefix - off) return 4;
      for (uint32_t b = 0; b < width; ++b) head[off + b] = (unsigned char)(value >> (8 * b));
    }
    // the file as a reader: the edited prefix, then the base's bytes, `file_len` bytes in all
    uint64_t pos = 0;
    auto rd = [&](void* dst, size_t bytes) {
      if (pos > file_len || bytes > file_len - pos) return false;
      unsigned char* d = static_cast<unsigned char*>(dst);
      for (size_t i = 0; i < bytes; ++i, ++pos) d[i] = pos < prefix ? head[pos] : base[pos];
      return true;
    };
    EngineTables t;
    Verdict v = read_engine_tables(rd, &t);
    if (v.ok()) v = validate_engine(t.h, t.bufs.data(), t.ops.data(), file_len - pos);
    const int32_t rec[2] = {(int32_t)id, (int32_t)v.code};
    if (fwrite(rec, sizeof rec, 1, out) != 1) return 5;
    printf("%u %d %s\n", id, v.code, v.msg);
    free(head);
  }
  if (c.left) return 4;
  free(in);
  if (fclose(out)) return 5;
  return 0;
}
