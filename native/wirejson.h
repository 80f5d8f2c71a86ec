/* wirejson: JSON to and from bytes for the wire path (see wirejson.c). */
#ifndef AM_WIREJSON_H
#define AM_WIREJSON_H

#define PY_SSIZE_T_CLEAN
#include <Python.h>

/* number of slots in the decoder's direct-mapped key cache; a key's slot is
 * FNV-1a (32 bit) over its bytes, modulo this */
#define AM_KEY_CACHE_SLOTS 2048
#define AM_KEY_CACHE_MAX_LEN 32

PyObject *am_json_dumpb(PyObject *self, PyObject *obj);
PyObject *am_json_frame(PyObject *self, PyObject *const *args, Py_ssize_t nargs);
PyObject *am_json_loadb(PyObject *self, PyObject *data);

#endif
