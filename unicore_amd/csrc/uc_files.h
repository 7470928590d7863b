// uc_files.h — what the file levels of the modules behind `cluster` share (uc_profile_host.cpp, uc_msa_host.cpp): the exception boundary of an
// entry point, whitespace as Rust's split_whitespace sees ASCII, whole-file writes and `create_dir_all`.
#pragma once
#include <sys/stat.h>

#include <cstdio>
#include <new>
#include <string>

#include "uc_common.h"

namespace uc {

template <typename F>
int guard(F &&f) {
    try {
        f();
        return UC_OK;
    } catch (const Error &e) {
        set_last_error(e.what());
        return e.code;
    } catch (const std::bad_alloc &) {
        set_last_error("out of host memory");
        return UC_ERR_GENERIC;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return UC_ERR_GENERIC;
    }
}

inline bool is_space(char c) { return c == ' ' || (c >= '\t' && c <= '\r'); }

inline void write_file(const std::string &path, const std::string &content) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) fail(UC_ERR_IO, "cannot write %s", path.c_str());
    const bool ok = fwrite(content.data(), 1, content.size(), f) == content.size();
    if (fclose(f) != 0 || !ok) fail(UC_ERR_IO, "cannot write %s", path.c_str());
}

inline void make_dirs(const std::string &path) {      // profile.rs:158-160, tree.rs:31-33
    std::string cur;
    for (size_t i = 0; i <= path.size(); i++) {
        if ((i == path.size() || path[i] == '/') && !cur.empty() && cur != "/") {
            struct stat st;
            if (stat(cur.c_str(), &st) != 0 && mkdir(cur.c_str(), 0777) != 0 && stat(cur.c_str(), &st) != 0) fail(UC_ERR_IO, "cannot create directory %s", cur.c_str());
        }
        if (i < path.size()) cur.push_back(path[i]);
    }
}

}  // namespace uc
