#include "hdf5_writer.hpp"

#include <dlfcn.h>

#include <cstdint>
#include <cstdlib>

#include "base.hpp"

namespace nvsm_host {
namespace {

// The handful of HDF5 1.10+ C entry points the writer needs (hid_t is int64_t since 1.10), declared here instead
// of pulling a foreign include directory into the build.
typedef int64_t hid_t;
typedef int herr_t;
typedef unsigned long long hsize_t;
constexpr unsigned kH5F_ACC_EXCL = 0x0004u, kH5F_ACC_RDONLY = 0x0000u;
constexpr int kH5T_FLOAT = 1;          // H5T_class_t
constexpr hid_t kH5P_DEFAULT = 0, kH5S_ALL = 0;
constexpr int kH5T_ORDER_LE = 0;

struct Hdf5Api {
    void* handle = nullptr;
    herr_t (*open)() = nullptr;
    herr_t (*get_libversion)(unsigned*, unsigned*, unsigned*) = nullptr;
    hid_t (*Fcreate)(const char*, unsigned, hid_t, hid_t) = nullptr;
    herr_t (*Fclose)(hid_t) = nullptr;
    hid_t (*Screate_simple)(int, const hsize_t*, const hsize_t*) = nullptr;
    herr_t (*Sclose)(hid_t) = nullptr;
    hid_t (*Tcopy)(hid_t) = nullptr;
    herr_t (*Tset_order)(hid_t, int) = nullptr;
    herr_t (*Tclose)(hid_t) = nullptr;
    hid_t (*Dcreate2)(hid_t, const char*, hid_t, hid_t, hid_t, hid_t, hid_t) = nullptr;
    herr_t (*Dwrite)(hid_t, hid_t, hid_t, hid_t, hid_t, const void*) = nullptr;
    herr_t (*Dclose)(hid_t) = nullptr;
    herr_t (*Eset_auto2)(hid_t, void*, void*) = nullptr;
    // ... and what read_hdf5 needs
    hid_t (*Fopen)(const char*, unsigned, hid_t) = nullptr;
    int (*Lexists)(hid_t, const char*, hid_t) = nullptr;                  // htri_t
    hid_t (*Dopen2)(hid_t, const char*, hid_t) = nullptr;
    hid_t (*Dget_space)(hid_t) = nullptr;
    hid_t (*Dget_type)(hid_t) = nullptr;
    int (*Sget_simple_extent_ndims)(hid_t) = nullptr;
    int (*Sget_simple_extent_dims)(hid_t, hsize_t*, hsize_t*) = nullptr;
    int (*Tget_class)(hid_t) = nullptr;
    size_t (*Tget_size)(hid_t) = nullptr;
    herr_t (*Dread)(hid_t, hid_t, hid_t, hid_t, hid_t, void*) = nullptr;
    hid_t* native_float = nullptr;

    static Hdf5Api& get() {
        static Hdf5Api api;
        if (api.handle) return api;
        std::vector<std::string> names;
        if (const char* env = std::getenv("NVSM_HDF5_LIB")) names.push_back(env);
        for (const char* n : {"libhdf5.so", "libhdf5_serial.so", "libhdf5.so.103", "libhdf5_serial.so.103", "/opt/conda/lib/libhdf5.so",
                              "/usr/lib/x86_64-linux-gnu/hdf5/serial/libhdf5.so", "/usr/lib/x86_64-linux-gnu/libhdf5_serial.so"})
            names.push_back(n);
        std::string tried;
        for (const std::string& n : names) {
            api.handle = dlopen(n.c_str(), RTLD_NOW | RTLD_LOCAL);
            if (api.handle) break;
            tried += n + " ";
        }
        if (!api.handle) NVSM_LOG(FATAL) << "cannot load libhdf5 (set NVSM_HDF5_LIB); tried: " << tried;
#define NVSM_H5_SYM(field, sym)                                                             \
        api.field = reinterpret_cast<decltype(api.field)>(dlsym(api.handle, sym));          \
        if (!api.field) NVSM_LOG(FATAL) << "libhdf5 lacks " << sym;
        NVSM_H5_SYM(open, "H5open") NVSM_H5_SYM(get_libversion, "H5get_libversion") NVSM_H5_SYM(Fcreate, "H5Fcreate")
        NVSM_H5_SYM(Fclose, "H5Fclose") NVSM_H5_SYM(Screate_simple, "H5Screate_simple") NVSM_H5_SYM(Sclose, "H5Sclose")
        NVSM_H5_SYM(Tcopy, "H5Tcopy") NVSM_H5_SYM(Tset_order, "H5Tset_order") NVSM_H5_SYM(Tclose, "H5Tclose")
        NVSM_H5_SYM(Dcreate2, "H5Dcreate2") NVSM_H5_SYM(Dwrite, "H5Dwrite") NVSM_H5_SYM(Dclose, "H5Dclose")
        NVSM_H5_SYM(Eset_auto2, "H5Eset_auto2") NVSM_H5_SYM(native_float, "H5T_NATIVE_FLOAT_g")
        NVSM_H5_SYM(Fopen, "H5Fopen") NVSM_H5_SYM(Lexists, "H5Lexists") NVSM_H5_SYM(Dopen2, "H5Dopen2") NVSM_H5_SYM(Dget_space, "H5Dget_space")
        NVSM_H5_SYM(Dget_type, "H5Dget_type") NVSM_H5_SYM(Sget_simple_extent_ndims, "H5Sget_simple_extent_ndims")
        NVSM_H5_SYM(Sget_simple_extent_dims, "H5Sget_simple_extent_dims") NVSM_H5_SYM(Tget_class, "H5Tget_class")
        NVSM_H5_SYM(Tget_size, "H5Tget_size") NVSM_H5_SYM(Dread, "H5Dread")
#undef NVSM_H5_SYM
        unsigned maj = 0, min = 0, rel = 0;
        api.get_libversion(&maj, &min, &rel);
        if (maj != 1 || min < 10) NVSM_LOG(FATAL) << "libhdf5 " << maj << "." << min << "." << rel << " found; 1.10 or newer is required";
        if (api.open() < 0) NVSM_LOG(FATAL) << "H5open failed";
        return api;
    }
};

}  // namespace

void hdf5_preload() { (void)Hdf5Api::get(); }

void write_hdf5(const std::string& filename, const std::vector<Hdf5Dataset>& datasets) {
    Hdf5Api& h5 = Hdf5Api::get();
    h5.Eset_auto2(0 /* H5E_DEFAULT */, nullptr, nullptr);      // errors are reported through return codes below
    const hid_t file = h5.Fcreate(filename.c_str(), kH5F_ACC_EXCL, kH5P_DEFAULT, kH5P_DEFAULT);
    if (file < 0) NVSM_LOG(FATAL) << "unable to create " << filename << " (H5F_ACC_EXCL: the file must not exist yet)";
    for (const Hdf5Dataset& d : datasets) {
        const hsize_t dims[2] = {d.rank == 1 ? d.dim0 * d.dim1 : d.dim0, d.dim1};
        const hid_t space = h5.Screate_simple(d.rank == 1 ? 1 : 2, dims, nullptr);
        const hid_t type = h5.Tcopy(*h5.native_float);
        bool ok = space >= 0 && type >= 0 && h5.Tset_order(type, kH5T_ORDER_LE) >= 0;
        hid_t dset = -1;
        if (ok) dset = h5.Dcreate2(file, d.name.c_str(), type, space, kH5P_DEFAULT, kH5P_DEFAULT, kH5P_DEFAULT);
        ok = ok && dset >= 0 && h5.Dwrite(dset, *h5.native_float, kH5S_ALL, kH5S_ALL, kH5P_DEFAULT, d.data) >= 0;
        if (dset >= 0) h5.Dclose(dset);
        if (type >= 0) h5.Tclose(type);
        if (space >= 0) h5.Sclose(space);
        if (!ok) { h5.Fclose(file); NVSM_LOG(FATAL) << "failed to write dataset " << d.name << " to " << filename; }
    }
    if (h5.Fclose(file) < 0) NVSM_LOG(FATAL) << "failed to close " << filename;
}

std::vector<Hdf5Array> read_hdf5(const std::string& filename, const std::vector<std::string>& names) {
    Hdf5Api& h5 = Hdf5Api::get();
    h5.Eset_auto2(0 /* H5E_DEFAULT */, nullptr, nullptr);
    const hid_t file = h5.Fopen(filename.c_str(), kH5F_ACC_RDONLY, kH5P_DEFAULT);
    if (file < 0) NVSM_LOG(FATAL) << "unable to open " << filename << " as an HDF5 file";
    std::vector<Hdf5Array> out;
    std::string error;
    for (const std::string& name : names) {
        if (h5.Lexists(file, name.c_str(), kH5P_DEFAULT) <= 0) { error = "holds no dataset " + name; break; }
        const hid_t dset = h5.Dopen2(file, name.c_str(), kH5P_DEFAULT);
        if (dset < 0) { error = "holds no dataset " + name; break; }
        const hid_t space = h5.Dget_space(dset), type = h5.Dget_type(dset);
        Hdf5Array a;
        a.name = name;
        hsize_t dims[2] = {0, 0};
        if (space < 0 || type < 0) error = "dataset " + name + " cannot be described";
        else if (h5.Sget_simple_extent_ndims(space) != 2) error = "dataset " + name + " is not two-dimensional";
        else if (h5.Tget_class(type) != kH5T_FLOAT || h5.Tget_size(type) != sizeof(float)) error = "dataset " + name + " does not hold float32 values";
        else if (h5.Sget_simple_extent_dims(space, dims, nullptr) != 2) error = "dataset " + name + " cannot be described";
        else {
            a.dim0 = dims[0]; a.dim1 = dims[1];
            a.data.resize(static_cast<size_t>(dims[0]) * static_cast<size_t>(dims[1]));
            if (!a.data.empty() && h5.Dread(dset, *h5.native_float, kH5S_ALL, kH5S_ALL, kH5P_DEFAULT, a.data.data()) < 0)
                error = "dataset " + name + " cannot be read";
        }
        if (type >= 0) h5.Tclose(type);
        if (space >= 0) h5.Sclose(space);
        h5.Dclose(dset);
        if (!error.empty()) break;
        out.push_back(std::move(a));
    }
    h5.Fclose(file);
    if (!error.empty()) NVSM_LOG(FATAL) << filename << " " << error;
    return out;
}

}  // namespace nvsm_host
