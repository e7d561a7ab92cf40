// Writes the vtable_*.ldb / vtable_*.vtb fixtures and vtable_cases.json: what
// the reference's own BuildTable (db/builder.cc) made of a MemTable's entries
// for several kv_sep_size and file numbers -- the table, the vTable, the
// VTableMeta, every entry's stored value -- and what its VTableReader::Get and
// VTableIndex::Decode say of good and of damaged handles, files and index
// values. The expectation tests/vtable_model.py is pinned against, and
// lvkv_vtable_*_device through it. TEST INFRASTRUCTURE; not part of the build.
// From the repository root, with the reference tree at $REF:
//
//   g++ -O2 -std=c++17 -DLEVELDB_PLATFORM_POSIX=1 -DLEVELDB_HAS_PORT_CONFIG_H=0 \
//       -DHAVE_SNAPPY=0 -DHAVE_ZSTD=0 -I$REF -I$REF/include -w -o /tmp/gen_vtable \
//       tests/golden/gen_vtable.cc \
//       $(ls $REF/util/*.cc $REF/table/*.cc $REF/db/*.cc | \
//         grep -v -e _test -e testutil -e env_windows -e leveldbutil -e /c.cc) -lpthread
//   /tmp/gen_vtable tests/golden
//
// An entry's input value is not written out: it is `first`, then len - 1 bytes
// of Pattern(seed) (below; tests/vtable_model.py restates it). The handle
// whose record_size_ passes its size is not run: the reference builds a Slice
// past its buffer there (table/vtable_format.cc:54).
#include <unistd.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "db/builder.h"
#include "db/dbformat.h"
#include "db/filename.h"
#include "db/memtable.h"
#include "db/table_cache.h"
#include "db/version_edit.h"
#include "leveldb/env.h"
#include "leveldb/filter_policy.h"
#include "leveldb/iterator.h"
#include "leveldb/options.h"
#include "table/vtable_format.h"
#include "table/vtable_manager.h"
#include "table/vtable_reader.h"

namespace {

using leveldb::Slice;
using leveldb::Status;

std::string out_dir, tmp_dir, json;
leveldb::Env* env;

std::string Hex(const Slice& s) {
  std::string out;
  char buf[4];
  for (size_t i = 0; i < s.size(); ++i) {
    snprintf(buf, sizeof buf, "%02x", static_cast<unsigned char>(s[i]));
    out += buf;
  }
  return out;
}

std::string Pattern(uint32_t seed, size_t n) {
  std::string s(n, '\0');
  for (size_t j = 0; j < n; ++j) s[j] = static_cast<char>((seed * 131u + j * 7u + (j >> 8)) & 0xffu);
  return s;
}

void Die(const std::string& what) {
  fprintf(stderr, "gen_vtable: %s\n", what.c_str());
  exit(1);
}

std::string ReadAll(const std::string& path) {
  std::string data;
  if (!leveldb::ReadFileToString(env, path, &data).ok()) Die("cannot read " + path);
  return data;
}

void WriteAll(const std::string& path, const std::string& data) {
  if (!leveldb::WriteStringToFile(env, data, path).ok()) Die("cannot write " + path);
}

struct In {
  std::string user_key;
  uint64_t seq;
  int type;  // 1 value, 0 deletion
  int first;
  size_t len;  // the whole value
  uint32_t seed;
  std::string value() const {
    if (len == 0) return std::string();
    return std::string(1, static_cast<char>(first)) + Pattern(seed, len - 1);
  }
};

// One VTableReader::Get on `path`: ,"status":..,"key":..,"value":..
std::string GetJson(const std::string& path, uint64_t number, uint64_t off, uint64_t size,
                    bool with_value) {
  leveldb::Options o;
  o.env = env;
  leveldb::VTableReader reader(number, nullptr);
  if (!reader.Open(o, path).ok()) Die("cannot open " + path);
  leveldb::VTableHandle h;
  h.offset = off;
  h.size = size;
  leveldb::VTableRecord rec;
  const Status s = reader.Get(h, &rec);
  std::string text = s.ToString();  // (an IO error names the file: without the directory)
  for (size_t at; (at = text.find(tmp_dir)) != std::string::npos;) text.erase(at, tmp_dir.size());
  std::string j = "\"off\":" + std::to_string(off) + ",\"size\":" + std::to_string(size) +
                  ",\"status\":\"" + text + "\"";
  if (s.ok()) {
    j += ",\"key\":\"" + Hex(rec.key) + "\",\"value_len\":" + std::to_string(rec.value.size());
    if (with_value) j += ",\"value\":\"" + Hex(rec.value) + "\"";
  }
  reader.Close();
  return j;
}

std::string last_vtb_path;  // a vTable BuildTable wrote, for the damaged handles
uint64_t last_vtb_number;
std::string an_index;       // an index value BuildTable stored

void Table(const std::string& name, uint64_t sep, uint64_t number, const std::vector<In>& ins,
           bool last) {
  leveldb::InternalKeyComparator icmp(leveldb::BytewiseComparator());
  const leveldb::FilterPolicy* bloom = leveldb::NewBloomFilterPolicy(10);
  leveldb::InternalFilterPolicy ipolicy(bloom);
  leveldb::Options o;
  o.env = env;
  o.comparator = &icmp;
  o.filter_policy = &ipolicy;
  o.compression = leveldb::kNoCompression;
  o.kv_sep_size = sep;
  const std::string dbname = tmp_dir + "/" + name;
  env->CreateDir(dbname);
  leveldb::MemTable* mem = new leveldb::MemTable(icmp);
  mem->Ref();
  for (const In& in : ins)
    mem->Add(in.seq, static_cast<leveldb::ValueType>(in.type), in.user_key, in.value());
  leveldb::TableCache cache(dbname, o, 10);
  leveldb::FileMetaData meta;
  meta.number = number;
  leveldb::VTableMeta vmeta;
  vmeta.number = 0;
  vmeta.records_num = 0;
  vmeta.table_size = 0;
  leveldb::Iterator* it = mem->NewIterator();
  const Status s = leveldb::BuildTable(dbname, env, o, &cache, it, &meta, &vmeta);
  if (!s.ok()) Die(name + ": BuildTable: " + s.ToString());
  const std::string ldb = ReadAll(leveldb::TableFileName(dbname, number));
  WriteAll(out_dir + "/vtable_" + name + ".ldb", ldb);
  const std::string vtb_path = leveldb::VTableFileName(dbname, number);
  const bool has_vtb = env->FileExists(vtb_path);
  std::string vtb;
  if (has_vtb) {
    vtb = ReadAll(vtb_path);
    WriteAll(out_dir + "/vtable_" + name + ".vtb", vtb);
    if (vtb.size() != vmeta.table_size) Die(name + ": table_size is not the file's size");
  }
  json += "\"" + name + "\":{\"kv_sep_size\":" + std::to_string(sep) + ",\"file_number\":" +
          std::to_string(number) + ",\"ldb\":\"vtable_" + name + ".ldb\",\"vtb\":" +
          (has_vtb ? "\"vtable_" + name + ".vtb\"" : std::string("null")) +
          ",\"records_num\":" + std::to_string(vmeta.records_num) + ",\"table_size\":" +
          std::to_string(vmeta.table_size) + ",\"ldb_size\":" + std::to_string(meta.file_size) +
          ",\"entries\":[\n";
  // the memtable's order is the table's: walk both
  leveldb::Iterator* tit = cache.NewIterator(leveldb::ReadOptions(), number, meta.file_size);
  tit->SeekToFirst();
  bool first_entry = true;
  for (it->SeekToFirst(); it->Valid(); it->Next(), tit->Next()) {
    if (!tit->Valid() || tit->key() != it->key()) Die(name + ": the table's keys differ");
    const In* in = nullptr;
    leveldb::ParsedInternalKey p;
    leveldb::ParseInternalKey(it->key(), &p);
    for (const In& c : ins)
      if (Slice(c.user_key) == p.user_key && c.seq == p.sequence) in = &c;
    if (in == nullptr || Slice(in->value()) != it->value()) Die(name + ": lost an entry");
    const Slice stored = tit->value();
    const bool moved = it->value().size() >= sep;
    json += std::string(first_entry ? "" : ",\n") + "{\"k\":\"" + Hex(it->key()) +
            "\",\"first\":" + std::to_string(in->first) + ",\"len\":" + std::to_string(in->len) +
            ",\"seed\":" + std::to_string(in->seed) + ",\"moved\":" + (moved ? "true" : "false");
    first_entry = false;
    if (!moved) {
      if (stored != it->value()) Die(name + ": an entry that stays changed");
    } else {
      json += ",\"stored\":\"" + Hex(stored) + "\"";
      leveldb::VTableIndex index;
      Slice input = stored;
      const Status ds = index.Decode(&input);
      if (!ds.ok() || !input.empty() || index.file_number != number) Die(name + ": index");
      json += ",\"get\":{" + GetJson(vtb_path, number, index.vtable_handle.offset,
                                     index.vtable_handle.size, false) + "}";
      // (the record is the user key and the value without its first byte)
      leveldb::Options ro;
      ro.env = env;
      leveldb::VTableReader reader(number, nullptr);
      reader.Open(ro, vtb_path);
      leveldb::VTableRecord rec;
      if (!reader.Get(index.vtable_handle, &rec).ok() || rec.key != p.user_key ||
          rec.value != Slice(in->value().substr(1)))
        Die(name + ": record");
      reader.Close();
      an_index = stored.ToString();
    }
    json += "}";
  }
  if (tit->Valid()) Die(name + ": the table has more entries");
  delete tit;
  delete it;
  mem->Unref();
  json += "]}";
  json += last ? "\n" : ",\n";
  if (has_vtb) {
    last_vtb_path = vtb_path;
    last_vtb_number = number;
  }
  delete bloom;
}

std::string Fixed32(uint32_t v) {
  std::string s(4, '\0');
  for (int k = 0; k < 4; ++k) s[k] = static_cast<char>(v >> (8 * k));
  return s;
}

int ncrafted = 0;
// A file of our own, read by the reference: {"file":hex,"name":..,Get's fields}
void Crafted(const std::string& name, const std::string& file, uint64_t off, uint64_t size,
             bool last = false) {
  const std::string path = tmp_dir + "/crafted" + std::to_string(ncrafted++) + ".vtb";
  WriteAll(path, file);
  json += "{\"name\":\"" + name + "\",\"file\":\"" + Hex(file) + "\"," +
          GetJson(path, 9, off, size, true) + "}" + (last ? "\n" : ",\n");
}

void IndexCase(const std::string& name, const std::string& value, bool last = false) {
  leveldb::VTableIndex index;
  Slice input = value;
  const Status s = index.Decode(&input);
  json += "{\"name\":\"" + name + "\",\"value\":\"" + Hex(value) + "\",\"status\":\"" +
          s.ToString() + "\"";
  if (s.ok())
    json += ",\"file_number\":" + std::to_string(index.file_number) + ",\"off\":" +
            std::to_string(index.vtable_handle.offset) + ",\"size\":" +
            std::to_string(index.vtable_handle.size) + ",\"left\":" + std::to_string(input.size());
  json += std::string("}") + (last ? "\n" : ",\n");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) Die("usage: gen_vtable <output directory>");
  out_dir = argv[1];
  env = leveldb::Env::Default();
  char tmpl[] = "/tmp/gen_vtable_XXXXXX";
  if (mkdtemp(tmpl) == nullptr) Die("mkdtemp");
  tmp_dir = tmpl;

  json = "{\"tables\":{\n";
  {  // kv_sep_size 1: everything but the empty values moves
    std::vector<In> ins = {
        {"", 9, 1, 2, 1, 1},                      // user key of 0 bytes, stripped length 0
        {"a", 8, 1, 2, 2, 2},                     // 1 byte, kv_sep_size + 1
        {"a", 7, 0, 0, 0, 0},                     // a deletion: stays (0 < 1)
        {std::string(127, 'k'), 6, 1, 2, 128, 3},  // stripped 127
        {std::string(128, 'k'), 5, 1, 2, 129, 4},  // stripped 128
        {"first_is_1", 4, 1, 1, 40, 5},           // a moved value whose first byte is 1
        {"first_is_0", 3, 1, 0, 9, 6},
        {"first_is_255", 2, 1, 255, 3, 7},
        {"empty_value", 1, 1, 0, 0, 0},           // kv_sep_size - 1: stays
    };
    Table("sep1", 1, 7, ins, false);
  }
  {  // kv_sep_size 16, file number 128: offsets cross 128 and 16384
    std::vector<In> ins;
    uint64_t seq = 1000;
    for (int i = 0; i < 40; ++i) {
      char key[16];
      snprintf(key, sizeof key, "key%04d", i);
      const size_t len = i % 5 == 0 ? 15 : i % 5 == 1 ? 16 : i % 5 == 2 ? 17 : 150 + i;
      ins.push_back({key, seq--, 1, 2, len, static_cast<uint32_t>(100 + i)});
    }
    ins.push_back({"key0007", 2000, 0, 0, 0, 0});  // a deletion over a moved value
    ins.push_back({"key0050", seq--, 1, 2, 16384, 50});  // stripped 16383
    ins.push_back({"key0051", seq--, 1, 2, 16385, 51});  // stripped 16384
    for (int i = 60; i < 66; ++i) {
      char key[16];
      snprintf(key, sizeof key, "key%04d", i);
      ins.push_back({key, seq--, 1, i == 62 ? 1 : 2, static_cast<size_t>(20 + i), static_cast<uint32_t>(i)});
    }
    Table("sep16", 16, 128, ins, false);
  }
  {  // the default kv_sep_size, a file number of 6 varint bytes
    std::vector<In> ins = {
        {"big0", 30, 1, 2, 999, 21},  {"big1", 29, 1, 2, 1000, 22}, {"big2", 28, 1, 2, 1001, 23},
        {"big3", 27, 1, 2, 3000, 24}, {"small0", 26, 1, 2, 1, 25},  {"small1", 25, 1, 2, 100, 26},
        {"small1", 24, 0, 0, 0, 0},   {"small2", 23, 1, 1, 1200, 27},
    };
    Table("sep1000", 1000, uint64_t{1} << 35, ins, false);
  }
  {  // nothing moves: BuildTable removes the vTable
    std::vector<In> ins = {
        {"a", 3, 1, 2, 2000, 31}, {"b", 2, 1, 1, 10, 32}, {"c", 1, 0, 0, 0, 0},
    };
    Table("none", uint64_t{1} << 40, 7, ins, true);
  }
  json += "},\n";

  // damaged handles on a file BuildTable wrote
  const uint64_t F = ReadAll(last_vtb_path).size();
  json += "\"handles\":{\"table\":\"sep1000\",\"cases\":[\n";
  const uint64_t hs[][2] = {{0, 0}, {0, 3}, {F, 0}, {F, 5}, {F - 2, 2}, {F - 2, 5}, {F + 10, 0},
                            {F + 10, 8}, {0, F + 1}, {F - 1, 2}};
  const size_t nh = sizeof hs / sizeof hs[0];
  for (size_t i = 0; i < nh; ++i)
    json += "{" + GetJson(last_vtb_path, last_vtb_number, hs[i][0], hs[i][1], false) + "}" +
            (i + 1 < nh ? ",\n" : "\n");
  json += "]},\n";

  // files of our own
  json += "\"crafted\":[\n";
  const std::string good = std::string("\x03") + "abc" + "\x02" + "xy";  // 7 bytes
  Crafted("good", Fixed32(7) + good, 0, 11);
  Crafted("size_4_empty_record", Fixed32(0), 0, 4);
  Crafted("handle_longer_than_record", Fixed32(7) + good + "zz", 0, 13);
  Crafted("second_record", Fixed32(7) + good + Fixed32(7) + good, 11, 11);
  Crafted("length_smaller_than_contents", Fixed32(5) + good, 0, 11);
  Crafted("trailing_bytes", Fixed32(10) + good + "zzz", 0, 14);
  Crafted("key_varint_runs_out", Fixed32(1) + "\x80", 0, 5);
  Crafted("key_varint_five_bytes_on", Fixed32(6) + "\x80\x80\x80\x80\x80\x01", 0, 10);
  Crafted("value_varint_runs_out", Fixed32(5) + "\x03" + "abc" + "\x80", 0, 9);
  Crafted("key_passes_record", Fixed32(2) + "\x05" + "a", 0, 6);
  Crafted("value_passes_record", Fixed32(7) + "\x03" + "abc" + "\x09" + "xy", 0, 11);
  Crafted("no_value", Fixed32(4) + "\x03" + "abc", 0, 8);
  Crafted("empty_key_and_value", Fixed32(2) + std::string(2, '\0'), 0, 6);
  Crafted("non_canonical_lengths",
          Fixed32(10) + std::string("\x83\x00", 2) + "abc" + std::string("\x82\x80\x00", 3) + "xy", 0, 14);
  Crafted("varint32_high_bits_dropped",
          Fixed32(11) + "\x03" + "abc" + "\x82\x80\x80\x80\x10" + "xy", 0, 15, true);
  json += "],\n";

  // edited index values
  json += "\"index\":[\n";
  const std::string ix = an_index;  // byte 1, file number, offset, size
  if (ix.size() < 4 || ix[0] != 1) Die("no index value");
  IndexCase("good", ix);
  IndexCase("trailing_bytes", ix + "zz");
  for (int t : {0, 2, 3, 255}) IndexCase("type_" + std::to_string(t), std::string(1, static_cast<char>(t)) + ix.substr(1));
  IndexCase("empty", "");
  for (size_t n = 1; n < ix.size(); ++n) IndexCase("cut_to_" + std::to_string(n), ix.substr(0, n));
  const std::string max10 = std::string(9, '\xff') + "\x01";
  const std::string over10 = std::string(9, '\xff') + "\x7f";
  const std::string eleven = std::string(10, '\x80') + "\x01";
  IndexCase("number_10_bytes", "\x01" + max10 + "\x05\x06");
  IndexCase("number_10_bytes_high_bits", "\x01" + over10 + "\x05\x06");
  IndexCase("number_11_bytes", "\x01" + eleven + "\x05\x06");
  IndexCase("offset_10_bytes", std::string("\x01\x07") + max10 + "\x06");
  IndexCase("offset_11_bytes", std::string("\x01\x07") + eleven + "\x06");
  IndexCase("size_10_bytes", std::string("\x01\x07\x05") + max10);
  IndexCase("size_11_bytes", std::string("\x01\x07\x05") + eleven);
  IndexCase("number_cut_mid_varint", std::string("\x01\x80"));
  IndexCase("offset_cut_mid_varint", std::string("\x01\x07\x80"));
  IndexCase("size_cut_mid_varint", std::string("\x01\x07\x05\x80"));
  IndexCase("non_canonical", std::string("\x01\x87\x00\x85\x80\x00\x86\x00", 8), true);
  json += "]}\n";

  WriteAll(out_dir + "/vtable_cases.json", json);
  return 0;
}
