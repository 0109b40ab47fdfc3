// blackbox_mpc_amd._fastcall -- the host-in / host-out control step (bbmpc_optimize, bbmpc_optimize_gather) called from a
// CPython extension function instead of through ctypes.  What Engine.optimize did in Python on either side of the call --
// np.asarray, the shape test, np.copyto into a persistent array, seven arguments through libffi, three .copy() -- is
// strictly serial with the kernel: here the observation is read where it lies (float32) or cast into a scratch row
// (float64), the three results are allocated BEFORE the call and the library writes straight into them.
//
// The module does not link against libbbmpc.so: bind() is handed the addresses of the two entry points as integers (from
// the ctypes library object _lib.py already holds), so the library is loaded once, and a test can bind a stub.
// Plain CPython + NumPy C API on purpose: pybind11's dispatch costs about what ctypes costs.
//
// Anything that is not a C-contiguous float32 / float64 ndarray of shape exactly (A, S) with an index-like time step is
// answered with NotImplemented: Engine.optimize then runs its Python body, which raises today's errors.
#define PY_SSIZE_T_CLEAN
#include <Python.h>
#define NPY_NO_DEPRECATED_API NPY_1_7_API_VERSION
#include <numpy/arrayobject.h>

#include <cmath>
#include <cstdint>
#include <cstring>

namespace {

using optimize_fn = int (*)(void*, const float*, int32_t, int32_t, float*, float*, float*);
using gather_fn = int (*)(void*, const float*, int32_t, int32_t, float*, float*, float*, float*, int32_t);

struct Bound {
    PyObject_HEAD
    void* handle;
    optimize_fn optimize;
    gather_fn gather;
    npy_intp A, S, U;
};

constexpr npy_intp kStackFloats = 256;      // A * S up to here is converted on the stack (config 2: 3, cheetah: 20)

// The observation as the library wants it.  ready() == false after a successful parse means "not handled natively".
struct Observation {
    const float* data = nullptr;
    float* heap = nullptr;
    float stack[kStackFloats];
    ~Observation() { PyMem_Free(heap); }

    // 1: data points at A * S floats; 0: not a form the fast path takes; -1: a Python error is set
    int take(const Bound* b, PyObject* obj) {
        if (!PyArray_Check(obj)) return 0;
        PyArrayObject* a = (PyArrayObject*)obj;
        if (PyArray_NDIM(a) != 2 || PyArray_DIM(a, 0) != b->A || PyArray_DIM(a, 1) != b->S) return 0;
        if (!PyArray_IS_C_CONTIGUOUS(a) || !PyArray_ISALIGNED(a) || !PyArray_ISNOTSWAPPED(a)) return 0;
        const int type = PyArray_TYPE(a);
        if (type == NPY_FLOAT32) {
            data = (const float*)PyArray_DATA(a);
            return 1;
        }
        if (type != NPY_FLOAT64) return 0;
        const npy_intp n = b->A * b->S;
        float* dst = stack;
        if (n > kStackFloats) {
            dst = heap = (float*)PyMem_Malloc((size_t)n * sizeof(float));
            if (!heap) {
                PyErr_NoMemory();
                return -1;
            }
        }
        const double* src = (const double*)PyArray_DATA(a);
        for (npy_intp i = 0; i < n; ++i) {
            const float f = (float)src[i];              // the C cast np.copyto(..., casting="unsafe") applies
            // a finite double beyond float's range: NumPy warns ("overflow encountered in cast") -- leave it to NumPy
            if (std::isinf(f) && !std::isinf(src[i])) return 0;
            dst[i] = f;
        }
        data = dst;
        return 1;
    }
};

// 1: *out holds the value; 0: no __index__, or it does not fit (the Python body decides); -1: a Python error is set
int index_as_int64(PyObject* obj, int64_t* out) {
    if (!PyIndex_Check(obj)) return 0;
    PyObject* num = PyNumber_Index(obj);
    if (!num) return -1;
    int overflow = 0;
    const long long v = PyLong_AsLongLongAndOverflow(num, &overflow);
    Py_DECREF(num);
    if (overflow) return 0;
    if (v == -1 && PyErr_Occurred()) return -1;
    *out = (int64_t)v;
    return 1;
}

int index_as_int32(PyObject* obj, int32_t* out) {
    int64_t v = 0;
    const int rc = index_as_int64(obj, &v);
    if (rc != 1) return rc;
    if (v < INT32_MIN || v > INT32_MAX) return 0;
    *out = (int32_t)v;
    return 1;
}

// The three results, allocated before the library call: it writes straight into their memory.
struct Results {
    PyObject *action = nullptr, *next_state = nullptr, *reward = nullptr;
    ~Results() {
        Py_XDECREF(action);
        Py_XDECREF(next_state);
        Py_XDECREF(reward);
    }
    bool alloc(const Bound* b) {
        npy_intp au[2] = {b->A, b->U}, as[2] = {b->A, b->S}, a1[1] = {b->A};
        action = PyArray_SimpleNew(2, au, NPY_FLOAT32);
        next_state = action ? PyArray_SimpleNew(2, as, NPY_FLOAT32) : nullptr;
        reward = next_state ? PyArray_SimpleNew(1, a1, NPY_FLOAT32) : nullptr;
        return reward != nullptr;
    }
    float* ptr(PyObject* o) const { return (float*)PyArray_DATA((PyArrayObject*)o); }
    // the tuple on success, the library's code as an int otherwise (the caller runs _lib.check on it)
    PyObject* finish(int code) {
        if (code != 0) return PyLong_FromLong(code);
        return PyTuple_Pack(3, action, next_state, reward);
    }
};

PyObject* not_implemented() { Py_RETURN_NOTIMPLEMENTED; }

PyObject* bound_optimize(PyObject* self, PyObject* const* args, Py_ssize_t nargs) {
    const Bound* b = (const Bound*)self;
    if (nargs != 3) {
        PyErr_SetString(PyExc_TypeError, "optimize(state, t, add_noise) takes exactly three arguments");
        return nullptr;
    }
    Observation obs;
    int rc = obs.take(b, args[0]);
    if (rc <= 0) return rc ? nullptr : not_implemented();
    int32_t t = 0;
    rc = index_as_int32(args[1], &t);
    if (rc <= 0) return rc ? nullptr : not_implemented();
    const int noise = PyObject_IsTrue(args[2]);
    if (noise < 0) return nullptr;
    Results out;
    if (!out.alloc(b)) return nullptr;
    float *pa = out.ptr(out.action), *pn = out.ptr(out.next_state), *pr = out.ptr(out.reward);
    int code;
    Py_BEGIN_ALLOW_THREADS                   // as ctypes' CDLL does: several handles are driven from threads
    code = b->optimize(b->handle, obs.data, t, noise ? 1 : 0, pa, pn, pr);
    Py_END_ALLOW_THREADS
    return out.finish(code);
}

PyObject* bound_optimize_gather(PyObject* self, PyObject* const* args, Py_ssize_t nargs) {
    const Bound* b = (const Bound*)self;
    if (nargs != 5) {
        PyErr_SetString(PyExc_TypeError, "optimize_gather(state, d_gathered, slot, t, add_noise) takes exactly five arguments");
        return nullptr;
    }
    if (!b->gather) return not_implemented();
    Observation obs;
    int rc = obs.take(b, args[0]);
    if (rc <= 0) return rc ? nullptr : not_implemented();
    int64_t gathered = 0;
    rc = index_as_int64(args[1], &gathered);
    if (rc <= 0) return rc ? nullptr : not_implemented();
    int32_t slot = 0, t = 0;
    rc = index_as_int32(args[2], &slot);
    if (rc <= 0) return rc ? nullptr : not_implemented();
    rc = index_as_int32(args[3], &t);
    if (rc <= 0) return rc ? nullptr : not_implemented();
    const int noise = PyObject_IsTrue(args[4]);
    if (noise < 0) return nullptr;
    Results out;
    if (!out.alloc(b)) return nullptr;
    float *pa = out.ptr(out.action), *pn = out.ptr(out.next_state), *pr = out.ptr(out.reward);
    int code;
    Py_BEGIN_ALLOW_THREADS
    code = b->gather(b->handle, obs.data, t, noise ? 1 : 0, pa, pn, pr, (float*)(uintptr_t)gathered, slot);
    Py_END_ALLOW_THREADS
    return out.finish(code);
}

PyMethodDef bound_methods[] = {
    {"optimize", (PyCFunction)(void (*)(void))bound_optimize, METH_FASTCALL,
     "optimize(state, t, add_noise) -> (action [A,U], next_state [A,S], reward [A]) | error code | NotImplemented"},
    {"optimize_gather", (PyCFunction)(void (*)(void))bound_optimize_gather, METH_FASTCALL,
     "optimize_gather(state, d_gathered, slot, t, add_noise) -> the same"},
    {nullptr, nullptr, 0, nullptr}};

PyTypeObject BoundType = {PyVarObject_HEAD_INIT(nullptr, 0)};

PyObject* module_bind(PyObject*, PyObject* args) {
    unsigned long long handle = 0, fn_optimize = 0, fn_gather = 0;
    Py_ssize_t A = 0, S = 0, U = 0;
    if (!PyArg_ParseTuple(args, "KKKnnn:bind", &handle, &fn_optimize, &fn_gather, &A, &S, &U)) return nullptr;
    if (!fn_optimize || A < 1 || S < 1 || U < 1) {
        PyErr_SetString(PyExc_ValueError, "bind(handle, fn_optimize, fn_gather, A, S, U): fn_optimize and the sizes must be non-zero");
        return nullptr;
    }
    Bound* b = PyObject_New(Bound, &BoundType);
    if (!b) return nullptr;
    b->handle = (void*)(uintptr_t)handle;
    b->optimize = (optimize_fn)(uintptr_t)fn_optimize;
    b->gather = (gather_fn)(uintptr_t)fn_gather;
    b->A = A, b->S = S, b->U = U;
    return (PyObject*)b;
}

PyMethodDef module_methods[] = {
    {"bind", module_bind, METH_VARARGS,
     "bind(handle_addr, fn_optimize_addr, fn_gather_addr, A, S, U) -> object with optimize / optimize_gather"},
    {nullptr, nullptr, 0, nullptr}};

PyModuleDef module_def = {PyModuleDef_HEAD_INIT, "_fastcall", "native marshalling of the host-in / host-out control step", -1,
                          module_methods};

}  // namespace

PyMODINIT_FUNC PyInit__fastcall(void) {
    import_array();
    BoundType.tp_name = "blackbox_mpc_amd._fastcall.Bound";
    BoundType.tp_basicsize = sizeof(Bound);
    BoundType.tp_flags = Py_TPFLAGS_DEFAULT;
    BoundType.tp_doc = "bbmpc_optimize / bbmpc_optimize_gather of one engine handle";
    BoundType.tp_methods = bound_methods;
    if (PyType_Ready(&BoundType) < 0) return nullptr;
    return PyModule_Create(&module_def);
}
