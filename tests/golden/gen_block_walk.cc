// Writes block_walk.bin and block_walk.json: data blocks by the reference's
// BlockBuilder, seeded damaged copies of them, and for each what the
// reference's own Block + NewIterator(BytewiseComparator()) + SeekToFirst +
// Next until !Valid() yielded -- the keys, where each value lies in the block,
// and status().ToString(). The expectation tests/sst_entries_model.py is
// pinned against, and lvkv_sst_read_entries_device through it. TEST
// INFRASTRUCTURE; not part of the build. From the repository root, with the
// reference tree at $REF:
//
//   g++ -O2 -std=c++17 -DLEVELDB_PLATFORM_POSIX=1 -DLEVELDB_HAS_PORT_CONFIG_H=0 \
//       -I$REF -I$REF/include -w -o /tmp/gen_block_walk tests/golden/gen_block_walk.cc \
//       $REF/util/{crc32c,coding,comparator,options,status,env,env_posix,logging}.cc \
//       $REF/table/{block,block_builder,format,iterator}.cc -lpthread
//   /tmp/gen_block_walk tests/golden
//
// No case holds an entry whose non_shared + value_length wraps in 32 bits:
// DecodeEntry (table/block.cc:71) would let the reference read far outside
// the block. Safe() below walks every block first, with the sum taken
// exactly, and the generator stops rather than hand the reference one.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "leveldb/comparator.h"
#include "leveldb/iterator.h"
#include "leveldb/options.h"
#include "table/block.h"
#include "table/block_builder.h"
#include "table/format.h"

namespace {

typedef std::vector<std::pair<std::string, std::string>> Entries;

std::string bin, json;

std::string Build(int interval, const Entries& entries) {
  leveldb::Options o;
  o.block_restart_interval = interval;
  leveldb::BlockBuilder b(&o);
  for (const auto& e : entries) b.Add(e.first, e.second);
  return b.Finish().ToString();
}

uint32_t Fixed32(const std::string& s, size_t at) {
  uint32_t v = 0;
  for (int k = 3; k >= 0; --k) v = (v << 8) | static_cast<uint8_t>(s[at + k]);
  return v;
}

void PutFixed32(std::string* s, size_t at, uint32_t v) {
  for (int k = 0; k < 4; ++k) (*s)[at + k] = static_cast<char>(v >> (8 * k));
}

// Where the entries of an undamaged block end.
size_t Limit(const std::string& b) { return b.size() - 4 - 4 * Fixed32(b, b.size() - 4); }

// Entry offsets of an undamaged block whose varints all take one byte.
std::vector<size_t> Offsets(const std::string& b) {
  std::vector<size_t> out;
  for (size_t p = 0, limit = Limit(b); p < limit;) {
    out.push_back(p);
    if ((b[p] | b[p + 1] | b[p + 2]) & 128) abort();
    p += 3 + b[p + 1] + b[p + 2];
  }
  return out;
}

// `extra` put between the entries and the restart array.
std::string Insert(const std::string& b, const std::string& extra) {
  const size_t limit = Limit(b);
  return b.substr(0, limit) + extra + b.substr(limit);
}

// The walk's own arithmetic, exact: false when an entry it would decode has
// non_shared + value_length >= 2^32.
bool Safe(const std::string& b) {
  if (b.size() < 4) return true;
  const uint64_t nr = Fixed32(b, b.size() - 4);
  if (nr == 0 || nr > (b.size() - 4) / 4) return true;
  const uint64_t limit = b.size() - 4 - 4 * nr;
  uint64_t at = Fixed32(b, limit);
  while (at < limit) {
    if (limit - at < 3) return true;
    uint64_t v[3];
    for (int f = 0; f < 3; ++f) {
      v[f] = 0;
      int i = 0;
      for (;; ++i) {
        if (i == 5 || at >= limit) return true;
        const uint8_t c = b[at++];
        v[f] |= static_cast<uint64_t>(c & 127) << (7 * i);
        if (!(c & 128)) break;
      }
      v[f] &= 0xffffffffu;
    }
    if (v[1] + v[2] > 0xffffffffull) return false;
    if (limit - at < v[1] + v[2]) return true;
    at += v[1] + v[2];
  }
  return true;
}

void Case(const std::string& name, const std::string& block) {
  if (!Safe(block)) {
    fprintf(stderr, "%s: an entry whose 32-bit sum wraps\n", name.c_str());
    exit(1);
  }
  // (a copy of its own on the heap: an overrun would be the allocator's to see)
  std::unique_ptr<char[]> copy(new char[block.size() + 1]);
  block.copy(copy.get(), block.size());
  leveldb::BlockContents contents;
  contents.data = leveldb::Slice(copy.get(), block.size());
  contents.cachable = false;
  contents.heap_allocated = false;
  leveldb::Block b(contents);
  std::unique_ptr<leveldb::Iterator> it(b.NewIterator(leveldb::BytewiseComparator()));
  char buf[128];
  snprintf(buf, sizeof buf, "%s  {\"name\": \"%s\", \"offset\": %zu, \"size\": %zu, \"entries\": [",
           json.empty() ? "" : ",\n", name.c_str(), bin.size(), block.size());
  json += buf;
  bool first = true;
  for (it->SeekToFirst(); it->Valid(); it->Next()) {
    json += first ? "[\"" : ", [\"";
    first = false;
    const leveldb::Slice k = it->key();
    for (size_t i = 0; i < k.size(); ++i) {
      snprintf(buf, sizeof buf, "%02x", static_cast<uint8_t>(k[i]));
      json += buf;
    }
    snprintf(buf, sizeof buf, "\", %zu, %zu]",
             static_cast<size_t>(it->value().data() - copy.get()), it->value().size());
    json += buf;
  }
  json += "], \"status\": \"" + it->status().ToString() + "\"}";
  bin += block;
}

std::string Key(int i) {
  char buf[32];
  snprintf(buf, sizeof buf, "walk/key%04d", i * 7);
  return buf;
}

Entries Mixed(int n) {
  Entries e;
  for (int i = 0; i < n; ++i) e.push_back({Key(i), std::string(1 + (i * 5) % 9, 'a' + i % 26)});
  return e;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  const Entries mixed = Mixed(12);
  const std::string r1 = Build(1, mixed), r2 = Build(2, mixed), r16 = Build(16, mixed);

  // 1. untouched
  Case("clean_r1", r1);
  Case("clean_r2", r2);
  Case("clean_r16", r16);
  // 2. too short to hold a restart count, and just long enough
  Case("len0", "");
  Case("len3", std::string("\1\0\0", 3));
  Case("len4_count0", std::string(4, '\0'));
  Case("len4_count1", std::string("\1\0\0\0", 4));
  {  // 3. restart count 0 after entries: an empty iterator
    std::string b = r16.substr(0, Limit(r16)) + std::string(4, '\0');
    Case("count0", b);
  }
  {  // 4. one restart more than the length holds
    std::string b = r2;
    PutFixed32(&b, b.size() - 4, static_cast<uint32_t>((b.size() - 4) / 4 + 1));
    Case("count_too_many", b);
    b = r2;  // (the most it holds: the restart array swallows the entries)
    PutFixed32(&b, b.size() - 4, static_cast<uint32_t>((b.size() - 4) / 4));
    Case("count_most", b);
  }
  {  // 5. restart[0] elsewhere
    const std::vector<size_t> at = Offsets(r1);
    std::string b = r1;
    PutFixed32(&b, Limit(b), static_cast<uint32_t>(at[1]));
    Case("restart0_second_entry", b);
    b = r1;
    PutFixed32(&b, Limit(b), static_cast<uint32_t>(Limit(b)));
    Case("restart0_at_end", b);
    b = r1;
    PutFixed32(&b, Limit(b), static_cast<uint32_t>(Limit(b) + 9));
    Case("restart0_past_end", b);
    b = r1;
    PutFixed32(&b, Limit(b), static_cast<uint32_t>(at[0] + 4));
    Case("restart0_mid_entry", b);
    b = r16;  // an entry with shared != 0 first: refused
    PutFixed32(&b, Limit(b), static_cast<uint32_t>(Offsets(r16)[1]));
    Case("restart0_shared_entry", b);
  }
  {  // 6. restart[1..] are not the walk's business
    const std::vector<size_t> at = Offsets(r2);
    std::string b = r2;
    PutFixed32(&b, Limit(b) + 4, static_cast<uint32_t>(at[2] + 5));
    Case("restart1_mid_entry", b);
    b = r2;
    const uint32_t one = Fixed32(b, Limit(b) + 4), two = Fixed32(b, Limit(b) + 8);
    PutFixed32(&b, Limit(b) + 4, two);
    PutFixed32(&b, Limit(b) + 8, one);
    Case("restart_out_of_order", b);
    b = r2;
    PutFixed32(&b, Limit(b) + 8, 0xfffffff0u);
    Case("restart2_past_end", b);
  }
  {  // 7. a restart-point entry that shares two bytes: legal for the walk
    std::string b = r1;
    b[Offsets(r1)[3]] = 2;
    Case("restart_entry_shares", b);
  }
  {  // 8. shared one more than the previous key's length
    std::string b = r16;
    b[Offsets(r16)[4]] = static_cast<char>(Key(3).size() + 1);
    Case("shared_too_long", b);
    b = r16;  // (exactly the previous key's length: legal)
    b[Offsets(r16)[4]] = static_cast<char>(Key(3).size());
    Case("shared_whole_key", b);
  }
  // 9. a varint the limit cuts
  Case("varint_cut", Insert(r16, std::string("\x80\x80\x80", 3)));
  Case("varint_cut_second", Insert(r16, std::string("\x00\x81\x80\x80", 4)));
  // 10. a fifth byte with its high bit set
  Case("varint_five_high", Insert(r16, std::string("\x80\x80\x80\x80\x80\x01\x00\x00", 8)));
  // 11. stray bytes before the restart array
  Case("stray_one", Insert(r16, std::string(1, '\0')));
  Case("stray_two", Insert(r16, std::string(2, '\0')));
  {  // 12. the last value one byte longer than what is left; and exactly what is left
    std::string b = r16;
    b[Offsets(r16).back() + 2] += 1;
    Case("value_past_limit", b);
    b = Insert(r16, std::string(1, 'x'));
    b[Offsets(r16).back() + 2] += 1;
    Case("value_to_limit", b);
  }
  {  // 13. an empty key first; 14. an empty value
    Entries e = Mixed(5);
    e.insert(e.begin(), {"", "value-of-the-empty-key"});
    Case("empty_key_first", Build(2, e));
    e = Mixed(6);
    e[0].second.clear();
    e[3].second.clear();
    e[5].second.clear();
    Case("empty_values", Build(2, e));
  }
  {  // two-byte varints, a five-byte one that is legal
    Entries e;
    const std::string prefix(140, 'p');
    for (int i = 0; i < 4; ++i) e.push_back({prefix + Key(i), std::string(130 + i, 'v')});
    std::string b = Build(16, e);
    Case("two_byte_varints", b);
    // entry 0's shared (0) as five bytes, 80 80 80 80 00; restart[0] still says 0
    Case("five_byte_zero", std::string("\x80\x80\x80\x80", 4) + b);
  }

  FILE* f = fopen((dir + "/block_walk.bin").c_str(), "wb");
  fwrite(bin.data(), 1, bin.size(), f);
  fclose(f);
  f = fopen((dir + "/block_walk.json").c_str(), "w");
  fprintf(f, "{\"cases\": [\n%s\n]}\n", json.c_str());
  fclose(f);
  return 0;
}
