// javaser.hpp -- Java Object Serialization (ObjectOutputStream protocol 2)
// for the IPLS partial-update object, org.javatuples.Pair<Integer, double[]>
// (MyIPFSClass.Update_file(String, Pair), MyIPFSClass.java:160-166;
// Download_Partial_Updates, :326-338), and for the saved-model files further
// down (HashMap<Integer,double[]>, double[], ArrayList<Double>).  Host code
// inside libipls_agg.so.
#pragma once
#include <cstdint>
#include <vector>

namespace ipls {
namespace javaser {

// Layout of the stream for n doubles: [header][8n BE payload][trailer].
int64_t pair_header_len();
int64_t pair_trailer_len();
// Write the header (ends with the double[] length) / trailer; `out` holds
// pair_header_len() / pair_trailer_len() bytes.
void write_pair_header(uint8_t* out, int32_t workers, int32_t n);
void write_pair_trailer(uint8_t* out);

// Parse a Pair<Integer,double[]> stream.  Returns the number of doubles and
// sets *workers and *payload_off (byte offset of the first BE double), or -1
// for a malformed stream / other types.  Bounded by `n`; never reads past it.
int64_t parse_pair(const uint8_t* buf, int64_t n, int32_t* workers, int64_t* payload_off, const char** why);

// ---- saved-model files (JDK 8 ObjectOutputStream, handles from 0x7e0000) ----
//  MAP   HashMap<Integer,double[]>  IPLS.save_model (IPLS.java:1904-1911), read by
//        DownloadMapParameters (MyIPFSClass.java:559-566)
//  DARR  double[]                   _Upload_File(double[], ...) (MyIPFSClass.java:261-270)
//  DLIST ArrayList<Double>          the pid-5 `<ID>Model` reply and `<ID>ETHModel`
//        (IPLS.java:547-558, 2255-2273), read by DownloadParameters (MyIPFSClass.java:376-385)
// double[] payloads carry the raw bits (ObjectOutputStream.writeDoubles);
// Double.value goes through doubleToLongBits, so DLIST canonicalises NaN.
constexpr int64_t kSavedPrefixMax = 192;   // the longest framing before a payload (MAP entry 0: 181)
constexpr int64_t kDarrHeader = 27;        // DARR: payload offset
constexpr int64_t kDlistFirst = 129;       // DLIST: offset of the first value
constexpr int64_t kDlistRecord = 14;       // DLIST: 73 71 007e0002 + 8 value bytes per later element

// HashMap iteration order of the keys put in `parts` order (a key listed twice
// stays at its first position), with the table size and threshold
// HashMap.writeObject records (16 / 0 for the empty map).
void saved_shape(const int32_t* parts, int n_parts, std::vector<int32_t>& order, int32_t* buckets, int32_t* threshold);
// The framing bytes in front of one entry's payload: the stream header too when
// `first`.  out holds kSavedPrefixMax bytes; returns the count (181 / 20).
int64_t saved_entry_prefix(uint8_t* out, bool first, int32_t threshold, int32_t buckets, int32_t size, int32_t key,
                           int32_t len);
int64_t saved_empty(uint8_t* out);   // the 82 bytes of the empty map
int64_t darr_header(uint8_t* out, int32_t len);
// DLIST framing up to the first value (129 bytes; 57 for n == 0, then only 78)
int64_t dlist_header(uint8_t* out, int32_t n);
int64_t dlist_total(int64_t n);

// Parsers: exactly the shapes above, bounded by n, -1 with *why otherwise.
// parse_saved returns the entry count and fills the first max_entries rows of
// (key, array length, payload byte offset); duplicate keys are rejected.
// parse_darr returns the array length.  parse_dlist returns the element count
// after checking the header and the length arithmetic; the element records
// are checked where they are decoded.
int64_t parse_saved(const uint8_t* buf, int64_t n, int32_t* keys, int64_t* lens, int64_t* offs, int64_t max_entries,
                    const char** why);
int64_t parse_darr(const uint8_t* buf, int64_t n, int64_t* payload_off, const char** why);
int64_t parse_dlist(const uint8_t* buf, int64_t n, const char** why);

}  // namespace javaser
}  // namespace ipls
