/* Stand-in for OpenEXR's <ImfArray.h>: the reference includes it and uses nothing from it.  See ImfRgbaFile.h. */
#ifndef RPF_ORACLE_IMF_ARRAY_STAND_IN_H
#define RPF_ORACLE_IMF_ARRAY_STAND_IN_H
#endif
