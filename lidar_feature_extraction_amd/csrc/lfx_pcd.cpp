// lfx_pcd.cpp -- map files (PCD), on the host only: lfx_pcd_read, lfx_pcd_write (include/lfx.h).  Plain C++ with no HIP
// header: tests/test_map_files.py builds it on its own under AddressSanitizer and UndefinedBehaviorSanitizer.
#include "../../include/lfx.h"

#include <algorithm>
#include <cctype>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace
{

void say(char * msg, size_t msg_len, const std::string & text)
{
  if (!msg || msg_len == 0) {return;}
  const size_t n = text.size() < msg_len - 1 ? text.size() : msg_len - 1;
  std::memcpy(msg, text.data(), n);
  msg[n] = '\0';
}

struct File
{
  std::FILE * f = nullptr;
  ~File() {if (f) {std::fclose(f);}}
};

struct Field
{
  std::string name;
  uint64_t size = 0, count = 1;
  char type = 0;
  uint64_t offset = 0;                       // in a record (binary), or bytes of the fields before it per point (compressed)
  uint64_t values_before = 0;                // values of the fields before it (ascii)
};

std::vector<std::string> split(const std::string & line)
{
  std::vector<std::string> out;
  size_t i = 0;
  while (i < line.size()) {
    while (i < line.size() && std::isspace(static_cast<unsigned char>(line[i]))) {i++;}
    const size_t j = i;
    while (i < line.size() && !std::isspace(static_cast<unsigned char>(line[i]))) {i++;}
    if (i > j) {out.push_back(line.substr(j, i - j));}
  }
  return out;
}

bool to_u64(const std::string & s, uint64_t * v)
{
  if (s.empty() || s[0] == '-' || s[0] == '+') {return false;}
  errno = 0;
  char * end = nullptr;
  const unsigned long long x = std::strtoull(s.c_str(), &end, 10);
  if (errno != 0 || *end != '\0') {return false;}
  *v = x;
  return true;
}

bool to_f32(const char * b, const char * e, float * v)
{
  const std::string s(b, e);
  char * end = nullptr;
  *v = std::strtof(s.c_str(), &end);
  return end == s.c_str() + s.size() && !s.empty();
}

struct Header
{
  std::vector<Field> fields;
  uint64_t width = 0, height = 0, points = 0, record = 0, values = 0;
  bool has_width = false, has_height = false, has_points = false, has_count = false;
  std::string data;
  int ix[3] = {-1, -1, -1};
};

// the header up to and including the DATA line; `at` = the byte offset just behind it
int read_header(std::FILE * f, Header & h, uint64_t & at, std::string & why)
{
  std::vector<uint64_t> sizes, counts;
  std::vector<char> types;
  std::vector<std::string> names;
  std::string line;
  uint64_t line_no = 0;
  at = 0;
  for (;;) {
    line.clear();
    int ch = 0;
    bool any = false;
    while ((ch = std::fgetc(f)) != EOF) {
      any = true;
      at++;
      if (ch == '\n') {break;}
      line.push_back(static_cast<char>(ch));
      if (line.size() > (1u << 20)) {why = "header line " + std::to_string(line_no + 1) + " is longer than 1 MiB"; return LFX_ERR_FILE;}
    }
    if (!any) {why = "no DATA line in the header (end of file after " + std::to_string(line_no) + " lines)"; return LFX_ERR_FILE;}
    line_no++;
    if (!line.empty() && line.back() == '\r') {line.pop_back();}
    const std::vector<std::string> t = split(line);
    if (t.empty() || t[0][0] == '#') {continue;}
    const std::string & k = t[0];
    const std::string where = "header line " + std::to_string(line_no) + " (" + k + ")";
    if (k == "VERSION" || k == "VIEWPOINT") {
      continue;                              // (VIEWPOINT is not applied to the points: PCL does not either)
    } else if (k == "FIELDS") {
      names.assign(t.begin() + 1, t.end());
    } else if (k == "SIZE" || k == "COUNT") {
      std::vector<uint64_t> & v = k == "SIZE" ? sizes : counts;
      v.clear();
      for (size_t i = 1; i < t.size(); i++) {
        uint64_t x = 0;
        if (!to_u64(t[i], &x)) {why = where + ": '" + t[i] + "' is not a count"; return LFX_ERR_FILE;}
        v.push_back(x);
      }
      if (k == "COUNT") {h.has_count = true;}
    } else if (k == "TYPE") {
      types.clear();
      for (size_t i = 1; i < t.size(); i++) {
        if (t[i].size() != 1 || (t[i][0] != 'F' && t[i][0] != 'I' && t[i][0] != 'U')) {why = where + ": unknown type '" + t[i] + "'"; return LFX_ERR_FILE;}
        types.push_back(t[i][0]);
      }
    } else if (k == "WIDTH" || k == "HEIGHT" || k == "POINTS") {
      uint64_t x = 0;
      if (t.size() != 2 || !to_u64(t[1], &x)) {why = where + ": expected one count"; return LFX_ERR_FILE;}
      if (k == "WIDTH") {h.width = x; h.has_width = true;}
      if (k == "HEIGHT") {h.height = x; h.has_height = true;}
      if (k == "POINTS") {h.points = x; h.has_points = true;}
    } else if (k == "DATA") {
      if (t.size() != 2) {why = where + ": expected one kind"; return LFX_ERR_FILE;}
      h.data = t[1];
      if (h.data != "ascii" && h.data != "binary" && h.data != "binary_compressed") {why = where + ": unknown kind '" + h.data + "'"; return LFX_ERR_FILE;}
      break;
    }
    // (other keywords are skipped, as PCL's reader skips them)
  }
  const std::string head = "header (DATA at line " + std::to_string(line_no) + ")";
  if (names.empty()) {why = head + ": no FIELDS"; return LFX_ERR_FILE;}
  if (sizes.size() != names.size() || types.size() != names.size()) {why = head + ": SIZE and TYPE must give one entry per field"; return LFX_ERR_FILE;}
  if (!h.has_count) {counts.assign(names.size(), 1);}
  if (counts.size() != names.size()) {why = head + ": COUNT must give one entry per field"; return LFX_ERR_FILE;}
  if (!h.has_width || !h.has_height || !h.has_points) {why = head + ": WIDTH, HEIGHT and POINTS are required"; return LFX_ERR_FILE;}
  if (h.height != 0 && h.width > UINT64_MAX / h.height) {why = head + ": WIDTH x HEIGHT overflows"; return LFX_ERR_FILE;}
  if (h.points != h.width * h.height) {
    why = head + ": POINTS " + std::to_string(h.points) + " is not WIDTH x HEIGHT = " + std::to_string(h.width * h.height);
    return LFX_ERR_FILE;
  }
  for (size_t i = 0; i < names.size(); i++) {
    Field fd;
    fd.name = names[i];
    fd.size = sizes[i];
    fd.type = types[i];
    fd.count = counts[i];
    if (fd.size != 1 && fd.size != 2 && fd.size != 4 && fd.size != 8) {why = head + ": field '" + fd.name + "' has SIZE " + std::to_string(fd.size); return LFX_ERR_FILE;}
    if (fd.count == 0 || fd.count > (1u << 24)) {why = head + ": field '" + fd.name + "' has COUNT " + std::to_string(fd.count); return LFX_ERR_FILE;}
    fd.offset = h.record;
    fd.values_before = h.values;
    h.record += fd.size * fd.count;
    h.values += fd.count;
    h.fields.push_back(fd);
  }
  if (h.points && h.record > UINT64_MAX / h.points) {why = head + ": the data size overflows"; return LFX_ERR_FILE;}
  const char * xyz[3] = {"x", "y", "z"};
  for (int a = 0; a < 3; a++) {
    for (size_t i = 0; i < h.fields.size() && h.ix[a] < 0; i++) {
      if (h.fields[i].name == xyz[a]) {h.ix[a] = static_cast<int>(i);}
    }
    if (h.ix[a] < 0) {why = head + ": no field '" + xyz[a] + "'"; return LFX_ERR_UNSUPPORTED_FIELD;}
    const Field & fd = h.fields[h.ix[a]];
    if (fd.type != 'F' || fd.size != 4 || fd.count != 1) {
      why = head + ": field '" + fd.name + "' is TYPE " + fd.type + " SIZE " + std::to_string(fd.size) + " COUNT " +
        std::to_string(fd.count) + " (x, y and z must be F 4 1)";
      return LFX_ERR_UNSUPPORTED_FIELD;
    }
  }
  return LFX_OK;
}

// liblzf's lzf_decompress, bounds checked: false on any reference or run that leaves either buffer, or a short output
bool lzf_decode(const uint8_t * in, uint64_t in_len, uint8_t * out, uint64_t out_len, std::string & why, uint64_t base)
{
  uint64_t ip = 0, op = 0;
  while (ip < in_len) {
    const uint64_t at = ip;
    uint64_t ctrl = in[ip++];
    if (ctrl < 32) {
      ctrl++;
      if (ctrl > out_len - op) {why = "LZF literal run past the end of the output at byte " + std::to_string(base + at); return false;}
      if (ctrl > in_len - ip) {why = "LZF literal run past the end of the input at byte " + std::to_string(base + at); return false;}
      std::memcpy(out + op, in + ip, ctrl);
      op += ctrl;
      ip += ctrl;
    } else {
      uint64_t len = ctrl >> 5;
      uint64_t back = (ctrl & 31u) << 8;
      if (ip >= in_len) {why = "LZF reference cut off at byte " + std::to_string(base + at); return false;}
      if (len == 7) {
        len += in[ip++];
        if (ip >= in_len) {why = "LZF reference cut off at byte " + std::to_string(base + at); return false;}
      }
      back += in[ip++];
      back += 1;
      len += 2;
      if (back > op) {why = "LZF reference before the start of the output at byte " + std::to_string(base + at); return false;}
      if (len > out_len - op) {why = "LZF reference past the end of the output at byte " + std::to_string(base + at); return false;}
      for (uint64_t i = 0; i < len; i++, op++) {out[op] = out[op - back];}     // (overlapping copies byte by byte)
    }
  }
  if (op != out_len) {why = "LZF block decodes to " + std::to_string(op) + " bytes, the header says " + std::to_string(out_len); return false;}
  return true;
}

float f32_at(const uint8_t * p)
{
  float v;
  std::memcpy(&v, p, 4);                     // (little-endian files on a little-endian host)
  return v;
}

// one record into the output: counts non-finite ones, leaves them out when asked, writes only below the capacity
struct Sink
{
  float * points;
  uint64_t capacity, k = 0, nonfinite = 0;
  bool drop;
  void put(float x, float y, float z)
  {
    const bool finite = std::isfinite(x) && std::isfinite(y) && std::isfinite(z);
    if (!finite) {
      nonfinite++;
      if (drop) {return;}
    }
    if (k < capacity) {
      float * r = points + 4 * k;
      r[0] = x; r[1] = y; r[2] = z; r[3] = 1.0f;
    }
    k++;
  }
};

}  // namespace

extern "C" {

int lfx_pcd_read(const char * path, float * points, uint64_t capacity, int drop_nonfinite, uint64_t * n_points,
  uint64_t * n_nonfinite, char * msg, size_t msg_len)
{
  say(msg, msg_len, "");
  if (!path || !n_points) {say(msg, msg_len, "path and n_points are required"); return LFX_ERR_INVALID_ARGUMENT;}
  *n_points = 0;
  if (n_nonfinite) {*n_nonfinite = 0;}
  File file;
  file.f = std::fopen(path, "rb");
  if (!file.f) {say(msg, msg_len, std::string("cannot open ") + path + ": " + std::strerror(errno)); return LFX_ERR_FILE;}
  Header h;
  uint64_t at = 0;
  std::string why;
  int rc = read_header(file.f, h, at, why);
  if (rc != LFX_OK) {say(msg, msg_len, why); return rc;}
  if (!points) {*n_points = h.points; return LFX_OK;}
  // the data: the rest of the file
  std::vector<uint8_t> data;
  {
    uint8_t buf[1 << 16];
    size_t got = 0;
    while ((got = std::fread(buf, 1, sizeof(buf), file.f)) > 0) {data.insert(data.end(), buf, buf + got);}
    if (std::ferror(file.f)) {say(msg, msg_len, std::string("cannot read ") + path); return LFX_ERR_FILE;}
  }
  Sink out{points, capacity, 0, 0, drop_nonfinite != 0};
  const Field & fx = h.fields[h.ix[0]], & fy = h.fields[h.ix[1]], & fz = h.fields[h.ix[2]];
  if (h.data == "binary") {
    if (h.points && data.size() / h.points < h.record) {
      say(msg, msg_len, "binary data ends at byte " + std::to_string(at + data.size()) + ", " + std::to_string(h.points) +
          " records of " + std::to_string(h.record) + " bytes need " + std::to_string(at + h.points * h.record));
      return LFX_ERR_FILE;
    }
    for (uint64_t i = 0; i < h.points; i++) {
      const uint8_t * r = data.data() + i * h.record;
      out.put(f32_at(r + fx.offset), f32_at(r + fy.offset), f32_at(r + fz.offset));
    }
  } else if (h.data == "binary_compressed") {
    if (data.size() < 8) {say(msg, msg_len, "binary_compressed data cut off at byte " + std::to_string(at + data.size()) + " (no sizes)"); return LFX_ERR_FILE;}
    uint32_t sizes[2];
    std::memcpy(sizes, data.data(), 8);
    const uint64_t packed = sizes[0], unpacked = sizes[1];
    if (unpacked != h.points * h.record) {
      say(msg, msg_len, "binary_compressed uncompressed size " + std::to_string(unpacked) + " at byte " + std::to_string(at + 4) +
          " is not POINTS x record = " + std::to_string(h.points * h.record));
      return LFX_ERR_FILE;
    }
    if (packed > data.size() - 8) {
      say(msg, msg_len, "binary_compressed compressed size " + std::to_string(packed) + " at byte " + std::to_string(at) +
          " runs past the end of the file (" + std::to_string(data.size() - 8) + " bytes follow)");
      return LFX_ERR_FILE;
    }
    if (unpacked && !packed) {say(msg, msg_len, "binary_compressed compressed size 0 at byte " + std::to_string(at)); return LFX_ERR_FILE;}
    std::vector<uint8_t> soa(unpacked);
    if (unpacked && !lzf_decode(data.data() + 8, packed, soa.data(), unpacked, why, at + 8)) {say(msg, msg_len, why); return LFX_ERR_FILE;}
    // one field after another: field f's block starts at POINTS x (bytes of the fields before it per point)
    const uint8_t * px = soa.data() + h.points * fx.offset, * py = soa.data() + h.points * fy.offset, * pz = soa.data() + h.points * fz.offset;
    for (uint64_t i = 0; i < h.points; i++) {out.put(f32_at(px + 4 * i), f32_at(py + 4 * i), f32_at(pz + 4 * i));}
  } else {
    // ascii: one point per non-empty line, values separated by white space
    const char * p = reinterpret_cast<const char *>(data.data()), * end = p + data.size();
    uint64_t i = 0, line_at = at;
    while (i < h.points) {
      if (p >= end) {
        say(msg, msg_len, "ascii data ends at byte " + std::to_string(at + data.size()) + " after " + std::to_string(i) + " of " +
            std::to_string(h.points) + " points");
        return LFX_ERR_FILE;
      }
      const char * eol = static_cast<const char *>(std::memchr(p, '\n', static_cast<size_t>(end - p)));
      if (!eol) {eol = end;}
      float v[3] = {0.f, 0.f, 0.f};
      uint64_t tok = 0;
      const char * q = p;
      bool bad = false;
      while (q < eol) {
        while (q < eol && std::isspace(static_cast<unsigned char>(*q))) {q++;}
        if (q >= eol) {break;}
        const char * b = q;
        while (q < eol && !std::isspace(static_cast<unsigned char>(*q))) {q++;}
        for (int a = 0; a < 3; a++) {
          if (tok == h.fields[h.ix[a]].values_before && !to_f32(b, q, &v[a])) {bad = true;}
        }
        tok++;
      }
      if (tok != 0) {
        if (bad || tok != h.values) {
          say(msg, msg_len, "ascii point " + std::to_string(i) + " at byte " + std::to_string(line_at) + (bad ? ": a coordinate is not a number" :
              ": " + std::to_string(tok) + " values, the header gives " + std::to_string(h.values)));
          return LFX_ERR_FILE;
        }
        out.put(v[0], v[1], v[2]);
        i++;
      }
      line_at += static_cast<uint64_t>(eol - p) + 1;
      p = eol + 1;
    }
  }
  *n_points = out.k;
  if (n_nonfinite) {*n_nonfinite = out.nonfinite;}
  if (out.k > capacity) {
    say(msg, msg_len, "the file holds " + std::to_string(out.k) + " records, the capacity is " + std::to_string(capacity));
    return LFX_ERR_CAPACITY;
  }
  return LFX_OK;
}

int lfx_pcd_write(const char * path, const float * points, uint64_t n_points, char * msg, size_t msg_len)
{
  say(msg, msg_len, "");
  if (!path || !points) {say(msg, msg_len, "path and points are required"); return LFX_ERR_INVALID_ARGUMENT;}
  if (n_points == 0) {say(msg, msg_len, "an empty cloud is not written"); return LFX_ERR_INVALID_ARGUMENT;}
  if (n_points > UINT64_MAX / 16) {say(msg, msg_len, "too many points"); return LFX_ERR_INVALID_ARGUMENT;}
  const std::string n = std::to_string(n_points);
  const std::string head = "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z\nSIZE 4 4 4\nTYPE F F F\nCOUNT 1 1 1\n"
    "WIDTH " + n + "\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS " + n + "\nDATA binary\n";
  std::FILE * f = std::fopen(path, "wb");
  if (!f) {say(msg, msg_len, std::string("cannot open ") + path + " for writing: " + std::strerror(errno)); return LFX_ERR_FILE;}
  bool ok = std::fwrite(head.data(), 1, head.size(), f) == head.size();
  std::vector<float> buf;
  const uint64_t chunk = 1u << 16;
  for (uint64_t i = 0; ok && i < n_points; i += chunk) {
    const uint64_t m = n_points - i < chunk ? n_points - i : chunk;
    buf.resize(3 * m);
    for (uint64_t k = 0; k < m; k++) {std::memcpy(&buf[3 * k], points + 4 * (i + k), 12);}
    ok = std::fwrite(buf.data(), 12, m, f) == m;
  }
  ok = (std::fclose(f) == 0) && ok;
  if (!ok) {say(msg, msg_len, std::string("cannot write ") + path); return LFX_ERR_FILE;}
  return LFX_OK;
}

}  // extern "C"
