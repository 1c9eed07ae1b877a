# The units of beam_units.hip, walks_units.hip and build_units.hip: one object
# per unit, each compiled from the one source with -DMH_UNIT=<unit> (the sources
# say what a unit holds).  Included by the library's Makefile and tools/Makefile.units.
BEAM_UNITS := beam_a beam_b beam_c beam_d beam_x2a beam_x2b beam_x4a beam_x4b \
              beam_w1a beam_w1b beam_w2a beam_w2b beam_w4a beam_w4b beam_fa beam_fb beam_desc
WALKS_UNITS := walks_a walks_b walks_c walks_d
BUILD_UNITS := build_s34b build_s34d build_s34a build_s34c build_l34b build_l34d build_l34a build_l34c \
               build_s12d build_s12b build_d build_s12a build_s12c build_l12d build_l12b build_l12a build_l12c \
               build_a build_b build_c
