/* check_json: a Python interpreter with the extension's sources compiled in
 * under -fsanitize=address,undefined (`make native-check`). It behaves like
 * the python executable, with _amcore as a built-in module, and is run on
 * check_json.py, which drives the JSON corpus of
 * tests/unit/test_wirecodec_json.py through the sanitized codec.
 */
#define PY_SSIZE_T_CLEAN
#include <Python.h>

PyMODINIT_FUNC PyInit__amcore(void);

int
main(int argc, char **argv)
{
    if (PyImport_AppendInittab("_amcore", PyInit__amcore) < 0) {
        fprintf(stderr, "check_json: cannot register _amcore\n");
        return 1;
    }
    return Py_BytesMain(argc, argv);
}
