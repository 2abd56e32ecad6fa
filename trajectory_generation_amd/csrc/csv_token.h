// csv_token.h -- one non-empty CSV field [s, e) to a double on the host, the way the dataset reader takes it
// (dataset_csv.cpp traj_dataset_read_csv) and the way the device parser's declined fields are settled
// (traj_dataset_csv_token_host): std::from_chars; a literal past the double range gets the value Python's float() /
// pandas give it (+-inf, a signed zero or the nearest subnormal) from strtod; then the "nan" / "inf" spellings pandas
// may write; anything else is an error and *out is what from_chars left.  Host only (C++17 <charconv>).
#ifndef TGMPC_CSV_TOKEN_H
#define TGMPC_CSV_TOKEN_H

#include <charconv>
#include <cmath>
#include <cstdlib>
#include <string>
#include <system_error>

namespace tgcsv {

// true if the token is a number; false leaves an error for the caller to report
inline bool csv_token_f64(const char* s, const char* e, double* out) {
    auto res = std::from_chars(s, e, *out);
    if (res.ec == std::errc::result_out_of_range && res.ptr == e) {
        std::string tok(s, e);
        *out = std::strtod(tok.c_str(), nullptr);
    } else if (res.ec != std::errc() || res.ptr != e) {
        std::string tok(s, e);
        if (tok == "nan" || tok == "NaN") *out = NAN;
        else if (tok == "inf") *out = INFINITY;
        else if (tok == "-inf") *out = -INFINITY;
        else return false;
    }
    return true;
}

}  // namespace tgcsv

#endif
