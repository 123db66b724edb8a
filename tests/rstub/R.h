/* R.h of the R stand-in (tests/rstub): everything is declared in Rinternals.h. */
#ifndef RSTUB_R_H
#define RSTUB_R_H
#include "Rinternals.h"
#endif
